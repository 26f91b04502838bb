"""The fold step kernels of vimz_amd/csrc/r1cs_ops.hpp — k_fold_cross, k_fold5, k_fresh_cross_neg, k_count_unreduced, k_count_diff — restated in plain
Python integers, and the cases tests/test_gpu_fold_kernels.py runs them on.  Test infrastructure; no GPU here (tests/test_fold_ref_host.py checks this file).

The kernels skip their multiplications by WAVE ballots over the class of the fresh operand (mul_fresh: 0, 1, -1, anything), k_fold5 inside a divergent
branch, k_fold_cross skips the store to E lane by lane behind a second ballot.  So the data here is laid out by wave (64 consecutive elements: the block size
is a multiple of 64 and so is every grid stride), in three layouts:
  cycling   every fresh operand cycles the six fresh classes with a period of its own, the periods pairwise coprime: every pair of classes meets in a lane;
  uniform   every fresh operand of a whole wave is one of 0, 1, -1 (one class per wave and operand): no lane of such a wave needs the multiplication;
  generic   the uniform layout with ONE other value in one lane of each wave, at lane 0, 31, 32, 63 in turn, in one operand in turn.
The vector folded into E (Tin, minus r_prev·negB in the lookahead) is zero on whole waves, on all but one lane of a wave, and here and there."""
import random

from tests._seam_cases import FILL, cross_term, from_limbs, scalars, to_limbs      # noqa: F401  (re-exported for the tests)

R = 1 << 256
WAVE = 64
LAYOUTS = ("cycling", "uniform", "generic")
SIZES = (1, 63, 64, 65, 257, 333)
STRIDED = (1000, 1)                               # n and the forced grid: one block of 256 makes four passes, the last one partial
FRESH_CLASSES, RUNNING_CLASSES, SCALAR_CLASSES = 6, 4, 5
FRESH = ("az", "bz", "cz", "azn", "bzn", "czn")   # the six fresh operands of k_fold_cross; negB is the seventh mul_fresh operand
PERIODS = (7, 9, 13, 11, 8, 17, 19)               # of operand 0..5 in the order of FRESH, then negB: pairwise coprime; (az, bzn) meets every pair of
#                                                   classes within 7·8 = 56 lanes, (bz, azn) within 9·11 = 99
GENERIC_LANES = (0, 31, 32, 63)
NB = (0, 1, 37, "n-1", "n")


def mont(p, vals):
    """the words a vector holds on the device: v·2^256 mod p"""
    return [v * R % p for v in vals]


def fresh_value(p, cls, rng):
    return (0, 1, p - 1, 2, p - 2)[cls] if cls < 5 else rng.randrange(3, p - 2)


def running_value(p, cls, rng):
    return (0, 1, p - 1)[cls] if cls < 3 else rng.randrange(2, p - 1)


def scalar_classes(p, seed):
    """0, 1, p - 1, a 128-bit value (what a challenge of the product is) and a full-width one"""
    s = scalars(p, seed)
    return s[:3] + (random.Random(f"u128:{seed}").randrange(1 << 127, 1 << 128), s[3])


def is_unit(p, v):
    return v in (0, 1, p - 1)


def uniform_class(k, w):
    """the class (0, 1, -1) of fresh operand number k in wave w of the uniform layout"""
    return (w // 3) % 3 if k == 6 else (w * (1 + k % 2) + k // 2) % 3


def fresh_operands(p, layout, n, seed, names=FRESH, shift=0):
    """name -> n values; `names` are laid out as the operands 0, 1, .. of one kernel; shift: the uniform layout's classes start that many waves later"""
    rng = random.Random(f"fresh:{layout}:{n}:{seed}")
    out = {}
    for k, name in enumerate(names):
        kk = 6 if name == "negB" else k
        if layout == "cycling":
            out[name] = [fresh_value(p, (i % PERIODS[kk]) % FRESH_CLASSES, rng) for i in range(n)]
        else:
            out[name] = [fresh_value(p, uniform_class(kk, i // WAVE + shift), rng) for i in range(n)]
    if layout == "generic":
        for w in range((n + WAVE - 1) // WAVE):
            i = min(WAVE * w + GENERIC_LANES[w % 4], n - 1)
            out[names[w % len(names)]][i] = rng.randrange(3, p - 2)
    return out


def running_operands(p, n, seed, names=("AZ", "BZ", "CZ", "E")):
    rng = random.Random(f"running:{n}:{seed}")
    return {name: [running_value(p, rng.randrange(RUNNING_CLASSES), rng) for _ in range(n)] for name in names}


def tin_vector(p, layout, n, seed):
    """The cross term that arrives.  cycling: a running class per lane.  uniform / generic: wave w is all zero (w = 0 mod 3), zero but for one lane (1 mod 3)
    or a running class per lane (2 mod 3) — negB's class changes every three waves, so each kind of wave meets negB = 0, 1 and -1."""
    rng = random.Random(f"tin:{layout}:{n}:{seed}")
    if layout == "cycling":
        return [running_value(p, rng.randrange(RUNNING_CLASSES), rng) for _ in range(n)]
    out = []
    for i in range(n):
        w, lane = divmod(i, WAVE)
        if w % 3 == 0:
            out.append(0)
        elif w % 3 == 1:
            out.append(rng.randrange(2, p - 1) if lane == min(GENERIC_LANES[(w // 3) % 4], n - 1 - WAVE * w) else 0)
        else:
            out.append(running_value(p, rng.randrange(RUNNING_CLASSES), rng))
    return out


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------

def masked(p, t, a, azn, nb):
    """the vector the dense MSM takes (r1cs_ops.hpp, "The BOOLEAN-ROW form"): rows below nb in boolean-row form, t from nb on"""
    return [(2 * t[i] % p if azn[i] == 1 else 0 if azn[i] == 0 else (t[i] + a[i]) % p) if i < nb else t[i] for i in range(len(t))]


def fold_cross(p, AZ, BZ, CZ, E, Tin, fold_E, r, hasB, r_prev, negB, u1_new, az, bz, cz, out, azn, bzn, czn, u2, outm, nb):
    """The comment above k_fold_cross, literally.  out / outm: whether the vector is asked for.  Returns AZ, BZ, CZ, E, out (or None), outm (or None)."""
    n = len(AZ)
    a = [(AZ[i] + r * az[i]) % p for i in range(n)]
    b = [(BZ[i] + r * bz[i]) % p for i in range(n)]
    c = [(CZ[i] + r * cz[i]) % p for i in range(n)]
    e = list(E)
    if fold_E:
        e = [(E[i] + r * (Tin[i] - (r_prev * negB[i] if hasB else 0))) % p for i in range(n)]
    t = tm = None
    if out:
        t = [(a[i] * bzn[i] + b[i] * azn[i] - u1_new * czn[i] - c[i] * u2) % p for i in range(n)]
        if outm:
            tm = masked(p, t, a, azn, nb)
    return a, b, c, e, t, tm


def folded_vector(p, Tin, hasB, r_prev, negB):
    """what k_fold_cross folds into E: E must not be touched where this is zero"""
    return [(Tin[i] - (r_prev * negB[i] if hasB else 0)) % p for i in range(len(Tin))]


def fold5(p, groups, r):
    """groups: five (x1 or None, x2) pairs of equal length; x1 += r·x2, a group without x1 is skipped"""
    return [None if x1 is None else [(x + r * y) % p for x, y in zip(x1, x2)] for x1, x2 in groups]


def fresh_cross_neg(p, a0, b0, c0, a1, b1, c1):
    return [(c0[i] + c1[i] - a0[i] * b1[i] - a1[i] * b0[i]) % p for i in range(len(a0))]


def count_unreduced(p, raw):
    return sum(1 for x in raw if x >= p)


def count_diff(a, b):
    return sum(1 for x, y in zip(a, b) if x != y)


# ---- a chain of satisfied fresh rows (the relation test and the schedule) -----------------------------------------------------------------------------------

def satisfied_rows(p, n, rows, seed):
    """`rows` fresh instances (u = 1) with az∘bz = cz, az and bz from the fresh classes in the three layouts in turn, the wave classes of row k shifted by k waves so
    that two consecutive rows differ nearly everywhere (their fresh cross term negB is what the lookahead owes)"""
    out = []
    for k in range(rows):
        f = fresh_operands(p, LAYOUTS[k % 3], n, f"{seed}:row{k}", names=("az", "bz"), shift=k)
        out.append((f["az"], f["bz"], [x * y % p for x, y in zip(f["az"], f["bz"])]))
    return out


def direct_chain(p, rows, challenges):
    """The fold without any lookahead: from the zero instance (u = 0), step i folds row i with challenge r_i and the cross term T_i = cross_term(U_i, row i)
    (no error vector is folded at step 0: T_0 is zero).  Returns the list of states AFTER each step: dicts AZ, BZ, CZ, E, u and T (the cross term folded)."""
    n = len(rows[0][0])
    AZ, BZ, CZ, E, u = [0] * n, [0] * n, [0] * n, [0] * n, 0
    states = []
    for i, (az, bz, cz) in enumerate(rows):
        r = challenges[i]
        T = cross_term(p, AZ, BZ, CZ, u, az, bz, cz, 1)
        assert i > 0 or T == [0] * n
        AZ, BZ, CZ, E, _, _ = fold_cross(p, AZ, BZ, CZ, E, T, 1 if i else 0, r, 0, 0, None, 0, az, bz, cz, False, None, None, None, 1, False, 0)
        u = (u + r) % p
        states.append({"AZ": AZ, "BZ": BZ, "CZ": CZ, "E": E, "u": u, "T": T})
    return states


def schedule_plan(nrows):
    """What launch_fold_and_cross (vimz_amd/csrc/ivc.hip) does at each step of one call with the lookahead on and every row's negB at hand.  Two slots hold cross
    terms; step i reads slot i & 1 (slot 0 starts with step 0's, which is zero and is not folded).  Per step: fold_E; hasB — the slot was filled by a lookahead, so
    r_{i-1}·negB_i is still owed; need1 — row i + 1's cross term goes into the OTHER slot (no lookahead made it); look — row i + 2's goes into this slot: through
    k_fold_cross with out = Tin when need1 is off, as a k_cross_term pass of its own behind it when both are wanted (the first step)."""
    plan, slot_step, slot_hasB = [], [0, None], [False, False]
    for i in range(nrows):
        par = i & 1
        assert slot_step[par] == i
        fold_E = i > 0
        has_next = i + 1 < nrows
        st = {"i": i, "slot": par, "fold_E": fold_E, "hasB": fold_E and slot_hasB[par], "need1": has_next and slot_step[par ^ 1] != i + 1, "look": has_next and i + 2 < nrows}
        plan.append(st)
        if st["need1"]:
            slot_step[par ^ 1], slot_hasB[par ^ 1] = i + 1, False
        if st["look"]:
            slot_step[par], slot_hasB[par] = i + 2, True
    return plan


def run_schedule(p, rows, challenges, fold_cross_fn, fresh_cross_neg_fn, cross_term_fn):
    """Drives schedule_plan through three callables with the reference's signatures (the reference itself in tests/test_fold_ref_host.py, the hooks on the GPU) and
    yields after every step (step, AZ, BZ, CZ, E, the row whose cross term the step produced last or None, that cross term or None)."""
    n = len(rows[0][0])
    AZ, BZ, CZ, E, u = [0] * n, [0] * n, [0] * n, [0] * n, 0
    slots = [[0] * n, [FILL] * n]
    for st in schedule_plan(len(rows)):
        i, par = st["i"], st["slot"]
        az, bz, cz = rows[i]
        r, r_prev = challenges[i], challenges[i - 1] if i else 0
        negB = fresh_cross_neg_fn(p, *rows[i - 1], *rows[i]) if st["hasB"] else None
        u = (u + r) % p
        t = i + 1 if st["need1"] else i + 2 if st["look"] else None
        nxt = rows[t] if t is not None else (None, None, None)
        AZ, BZ, CZ, E, out, _ = fold_cross_fn(p, AZ, BZ, CZ, E, slots[par], int(st["fold_E"]), r, int(st["hasB"]), r_prev, negB, u, az, bz, cz,
                                              "separate" if st["need1"] else "alias" if st["look"] else False, *nxt, 1, False, 0)
        if st["need1"]:
            slots[par ^ 1] = out
            if st["look"]:
                t = i + 2
                out = slots[par] = cross_term_fn(p, AZ, BZ, CZ, u, *rows[t], 1)
        elif st["look"]:
            slots[par] = out
        yield st, AZ, BZ, CZ, E, t, out


# ---- raw patterns of the counting kernels ---------------------------------------------------------------------------------------------------------------

def _word(x, k):
    return (x >> (32 * k)) & 0xFFFFFFFF


def unreduced_patterns(p):
    """(name, raw 256-bit word, is it unreduced)"""
    out = [("zero", 0, False), ("p-1", p - 1, False), ("p", p, True), ("p+1", p + 1, True), ("max", R - 1, True)]
    assert _word(p, 0) != 0xFFFFFFFF and _word(p, 7) != 0xFFFFFFFF
    out.append(("p, word 0 raised", p - _word(p, 0) + 0xFFFFFFFF, True))
    out.append(("p, word 7 raised", p + (1 << 224), True))
    for k in (0, 3, 6):       # p - 1 with the top word one lower and a lower word raised to the full: the comparison must be decided by the top word
        x = p - 1 - (1 << 224)
        assert _word(x, 7) == _word(p, 7) - 1 and _word(x, k) != 0xFFFFFFFF
        x = x - (_word(x, k) << (32 * k)) + (0xFFFFFFFF << (32 * k))
        assert x < p and _word(x, k) > _word(p, k)
        out.append((f"below p, word {k} raised", x, False))
    return out


def diff_patterns(x):
    """(name, the other element, do they differ) for an element x"""
    return [("word 0", x ^ 1, True), ("word 7", x ^ (1 << 255), True), ("all words", x ^ (R - 1), True), ("none", x, False)]


COUNT_N = 130
COUNT_AT = (0, 63, 64, COUNT_N - 1)      # the first and the last element, both sides of a wave boundary


def count_cases(p, seed):
    """(what, name, a, b, n, expected): raw words; every pattern alone at every position among reduced random elements, all of them at once, and one just
    behind the counted range"""
    rng = random.Random(f"count:{seed}")
    base = [rng.randrange(p) for _ in range(COUNT_N + 1)]
    cases = [(0, "all reduced", base, None, COUNT_N, 0)]
    pats = unreduced_patterns(p)
    for name, x, bad in pats:
        for at in COUNT_AT:
            a = list(base); a[at] = x
            cases.append((0, f"{name} at {at}", a, None, COUNT_N, int(bad)))
    a = list(base)
    for k, (_, x, _) in enumerate(pats):
        a[(COUNT_AT + (1, 62, 65, 127, 128, 100))[k]] = x
    cases.append((0, "every pattern", a, None, COUNT_N, sum(1 for _, _, bad in pats if bad)))
    a = list(base); a[COUNT_N] = p
    cases.append((0, "p behind the range", a, None, COUNT_N, 0))
    cases.append((1, "equal", base, list(base), COUNT_N, 0))
    for k in range(4):
        for at in COUNT_AT:
            name, y, differ = diff_patterns(base[at])[k]
            b = list(base); b[at] = y
            cases.append((1, f"{name} at {at}", base, b, COUNT_N, int(differ)))
    b = list(base)
    for k, at in enumerate(COUNT_AT):
        b[at] = diff_patterns(base[at])[k][1]
    cases.append((1, "every pattern", base, b, COUNT_N, 3))
    b = list(base); b[COUNT_N] ^= 1
    cases.append((1, "a difference behind the range", base, b, COUNT_N, 0))
    for what, name, a, b, n, want in cases:      # the expectation is the reference's, not a second opinion
        assert want == (count_unreduced(p, a[:n]) if what == 0 else count_diff(a[:n], b[:n])), name
    return cases


# ---- case lists ----------------------------------------------------------------------------------------------------------------------------------------------

def sizes_and_grids():
    return [(n, 0) for n in SIZES] + [STRIDED]


def resolve_nb(sel, n):
    return min(n, {"n-1": n - 1, "n": n}.get(sel, sel))


E_MODES = ((0, 0), (0, 1), (1, 0), (1, 1))        # (fold_E, hasB); hasB without fold_E must change nothing
OUT_MODES = ("none", "separate", "alias")         # alias: out is the very vector passed as Tin


def _fold_cross_options():
    """The whole product of the options, (fold_E, hasB) fastest, then out, r_prev, outm / nb, u2, r.  An option the kernel cannot see in a combination — r_prev
    without fold_E and hasB, nb without an out — is left in: such combinations weigh the rarer settings (no out at all, hasB without fold_E) up.  u1_new takes
    the scalar class two behind r's."""
    opts = []
    for r in range(SCALAR_CLASSES):
        for u2 in (0, 1):
            for nbsel in (None,) + NB:
                for rp in range(SCALAR_CLASSES):
                    for o in OUT_MODES:
                        for fold_E, hasB in E_MODES:
                            opts.append({"fold_E": fold_E, "hasB": hasB, "r_prev": rp, "out": o, "nb": nbsel, "u2": u2, "r": r, "u1": (r + 2) % SCALAR_CLASSES})
    return opts


FOLD_CROSS_OPTIONS = _fold_cross_options()
# The pruning rule: the 3600 option combinations above are listed in that fixed order and every PRUNE-th one is kept, starting at a different place for every
# (layout, size).  PRUNE is a prime whose quotients by the running products of the options' value counts (4, 12, 60, 360, 720) are no multiples of the next
# count, so consecutive kept cases step every fast option.  BN254 Fr runs this for every layout and size, the other fields for the cycling layout with
# PRUNE_OTHER.  tests/test_fold_ref_host.py asserts what survives: every value of every option and every (fold_E, hasB, out) triple with every layout and size
# in Fr (every value with every size in the other fields), over a field's grid every (out, nb) and, in Fr, every (r, r_prev) pair of classes under the lookahead.
PRUNE, PRUNE_OTHER = 101, 199


def fold_cross_cases(fid):
    """(layout, n, blocks, options) for one field"""
    out = []
    combos = [(l, n, b) for l in (LAYOUTS if fid == 0 else LAYOUTS[:1]) for n, b in sizes_and_grids()]
    step = PRUNE if fid == 0 else PRUNE_OTHER
    for q, (layout, n, blocks) in enumerate(combos):
        for k in range((5 * q + fid) % step, len(FOLD_CROSS_OPTIONS), step):
            out.append((layout, n, blocks, FOLD_CROSS_OPTIONS[k]))
    return out


FOLD5_SHAPES = (      # (lengths, the group without x1, offsets of x1, offsets of x2): five different lengths, one of them 0; offsets not multiples of 64
    ((333, 0, 65, 1000, 257), 2, (1, 3, 65, 7, 130), (5, 2, 63, 9, 1)),
    ((1, 63, 64, 0, 130), 1, (67, 1, 2, 3, 5), (1, 66, 3, 2, 127)),       # the error vector's slot is the empty one at step 0
)
FOLD5_BLOCKS = (0, 1, 64)
FOLD5_SHARED = (3, 4)                      # these two groups' x1 are ranges of ONE vector, as the running products are ranges of one allocation


def fold5_cases():
    """(shape number, layout of x2, scalar class of r, blocks), for every field"""
    return [(s, l, r, b) for s in range(len(FOLD5_SHAPES)) for l in LAYOUTS for r in range(SCALAR_CLASSES) for b in FOLD5_BLOCKS]


FRESH_NEG_FIELDS = (0, 1)


def fresh_neg_cases():
    """(layout, n, blocks), for BN254 Fr and Fq"""
    return [(l, n, b) for l in LAYOUTS for n in SIZES + (STRIDED[0],) for b in (0, 1)]


SCHEDULE_N, SCHEDULE_ROWS = 333, 6
