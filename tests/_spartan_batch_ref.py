"""TEST INFRASTRUCTURE ONLY.  The batched compressed-proof verifier (vimz_amd/csrc/spartan_batch.hpp) in Python integers, on top of tests/_spartan_ref.py and
tests/_spartan_pub_ref.py: the matrix evaluation, an opening's s-vector with its index map (the shifted one too), the masked dot, the unrolled coefficients of an
opening's group equation, the accumulators and the batch equation.  Nothing here reads the library.  The group side goes through the CPU oracle (curve_mul,
curve_add, msm), as tests/_spartan.py does.

The unrolling:  ipa_verify's update P <- R + x·P + x²·L from P_0 = comm + claim·r0·U gives
    P_fin = (Π x)·comm + Σ_j (Π_{i>j} x_i)·(R_j + x_j²·L_j) + (Π x)·claim·r0·U,
and the opening holds iff  P_fin = afin·<s, G> + afin·bfin·r0·U,  s_i = Π_{bit p of i set} x_{rounds−1−p},  bfin = <s, b>.
The batch: under multipliers rho_o,  Σ_o rho_o·[Σ_k c_{o,k}·Q_{o,k}] + (Σ_o rho_o·g_o)·U = <acc, ck>,  acc[j] = Σ_o rho_o·afin_o·s_o[i] with j = i (an E opening) or
j = (i − 1) mod n (a W opening: index 0 sits on ck[n − 1], index i on ck[i − 1]).

Host test: tests/test_spartan_batch_ref_host.py; the GPU side: tests/_spartan_batch_gpu.py and tests/test_gpu_spartan_batch.py."""
import functools

import numpy as np

from tests import _spartan_pub_ref as P
from tests import _spartan_ref as S
from tests._oracle import CURVE_BASE, CURVE_SCALAR, ck_derive, to_limbs
from tests._spartan import Reader, Transcript, interp

GROUP = 4          # members one kernel pass serves (vimz_test_spartan_batch_group)
SPLIT_H = 10       # the half-table split (vimz_test_spartan_batch_split)
BLOCK_LOG2 = 8     # a workgroup has 256 threads


# ---- the field side ------------------------------------------------------------------------------------------------------------------------------------------
def mat_eval(case, rx, ry, w, p):
    """Σ_m w[m] Σ_(row, col, value) value·eq(rx, row)·eq(ry, col) over the triplets of `case` (repeated triplets are separate terms)"""
    ex, ey = S.eq_table(rx, p), S.eq_table(ry, p)
    return sum(wm * sum(v * ex[r] * ey[c] for r, c, v in case[m]) for m, wm in zip("ABC", w)) % p


def svec(xs, p):
    """s_i = the product of the challenges of the rounds in which index i sat in the right half: round 0 = the top bit"""
    s = [1]
    for x in reversed(xs):
        s = s + [v * x % p for v in s]
    return s


def slot_of(i, n, shifted):
    """the key point under index i of an opening over n slots"""
    return (i - 1) % n if shifted else i


def masked(i, n_pub, n_w):
    """k_mask_public's rule; n_w = 0: an E opening, nothing masked"""
    return n_w != 0 and (i == 0 or i + n_pub >= n_w)


def masked_dot(xs, pt, n_pub, n_w, p):
    s, b = svec(xs, p), S.eq_table(pt, p)
    return sum(si * bi for i, (si, bi) in enumerate(zip(s, b)) if not masked(i, n_pub, n_w)) % p


def dot_closed_form(xs, pt, p):
    """<s, eq(pt, ·)> of an E opening: both are tensor products"""
    out = 1
    for x, r in zip(xs, pt):
        out = out * ((1 - r) + x * r) % p
    return out


def unroll(xs, claim, r0, p):
    """(c_comm, [c_R_j], [c_L_j], g0)"""
    cR, cL, run = [0] * len(xs), [0] * len(xs), 1
    for j in reversed(range(len(xs))):
        cR[j], cL[j] = run, run * xs[j] * xs[j] % p
        run = run * xs[j] % p
    return run, cR, cL, run * claim * r0 % p


def _ipa_deferred(tr, comm, claim, rounds, rd, pb, ps, shifted, pt, n_pub, n_w):
    tr.fe(b"ipaP.x", comm[0]); tr.fe(b"ipaP.y", comm[1]); tr.fe(b"ipaC", claim)
    r0 = tr.challenge()
    Ls, Rs, xs = [], [], []
    for _ in range(rounds):
        L, R = rd.point(pb), rd.point(pb)
        tr.fe(b"L.x", L[0]); tr.fe(b"L.y", L[1]); tr.fe(b"R.x", R[0]); tr.fe(b"R.y", R[1])
        Ls.append(L); Rs.append(R); xs.append(tr.challenge())
    afin = rd.fe(ps)
    tr.fe(b"a", afin)
    c0, cR, cL, g0 = unroll(xs, claim, r0, ps)
    Q, c = [comm], [c0]
    for j in range(rounds):
        Q += [Rs[j], Ls[j]]; c += [cR[j], cL[j]]
    return {"shifted": shifted, "rounds": rounds, "xs": xs, "pt": list(pt), "n_pub": n_pub, "n_w": n_w, "afin": afin, "r0": r0, "g0": g0, "Q": Q, "c": c}


def deferred(cid, tr, digest, inst, n_w, n_c, side_tag, rd, has_E):
    """The host side of the deferred verifier for inst = (cW, cE, u, [X...]): a str — the scalar check that failed — or
    {"rx", "ry", "w", "claim", "vz", "openings": [W, E?]}; vm·vz == claim is left to the caller (the device computes vm)."""
    ps, pb = S.FIELD[CURVE_SCALAR[cid]], S.FIELD[CURVE_BASE[cid]]
    cW, cE, u, X = inst
    n_pub = len(X)
    if n_pub < 1 or n_w < n_pub + 2:
        return "shape"
    P._absorb_instance(tr, {"side_tag": side_tag, "digest": digest}, inst)
    s, t = (n_c - 1).bit_length(), (n_w - 1).bit_length()
    tau = [tr.challenge() for _ in range(s)]
    claim, rx = 0, []
    for _ in range(s):
        s0, s2, s3 = rd.fe(ps), rd.fe(ps), rd.fe(ps)
        tr.fe(b"o0", s0); tr.fe(b"o2", s2); tr.fe(b"o3", s3)
        rx.append(tr.challenge())
        claim = interp([s0, (claim - s0) % ps, s2, s3], rx[-1], ps)
    va, vb, vc, ve = rd.fe(ps), rd.fe(ps), rd.fe(ps), rd.fe(ps)
    if not has_E and ve != 0:
        return "E claim of a strict instance"
    e = 1
    for a_, b_ in zip(tau, rx):
        e = e * (a_ * b_ + (1 - a_) * (1 - b_)) % ps
    if e * (va * vb - u * vc - ve) % ps != claim:
        return "outer sum-check"
    for v in (va, vb, vc, ve):
        tr.fe(b"claim", v)
    rho = tr.challenge()
    claim, ry = (va + rho * vb + rho * rho * vc) % ps, []
    for _ in range(t):
        s0, s2 = rd.fe(ps), rd.fe(ps)
        tr.fe(b"i0", s0); tr.fe(b"i2", s2)
        ry.append(tr.challenge())
        claim = interp([s0, (claim - s0) % ps, s2], ry[-1], ps)
    evalW = rd.fe(ps)
    tr.fe(b"evalW", evalW)

    def eq_at(pt, idx):          # the product formula: no table
        out = 1
        for q, r in enumerate(pt):
            out = out * (r if (idx >> (len(pt) - 1 - q)) & 1 else 1 - r) % ps
        return out

    vz = (evalW + u * eq_at(ry, 0) + sum(x * eq_at(ry, n_w - n_pub + k) for k, x in enumerate(X))) % ps
    ops = [_ipa_deferred(tr, cW, evalW, t, rd, pb, ps, True, ry, n_pub, n_w)]
    if has_E:
        ops.append(_ipa_deferred(tr, cE, ve, s, rd, pb, ps, False, rx, 0, 0))
    return {"rx": rx, "ry": ry, "w": (1, rho, rho * rho % ps), "claim": claim, "vz": vz, "openings": ops}


def case_inst(c):
    """(u, [X...]) of a case of either module (those of _spartan_ref have two public elements)"""
    n_pub = c.get("n_pub", 2)
    return c["Z"][0], list(c["Z"][c["n_w"] - n_pub:])


def deferred_bytes(c, blob, label, u=None, X=None):
    """deferred() on cW ‖ cE ‖ argument as the provers of _spartan_ref / _spartan_pub_ref and the hooks write them; a str, or the dict with "trailing" added"""
    cid = c["cid"]
    pb = S.FIELD[CURVE_BASE[cid]]
    rd = Reader(blob)
    try:
        cW, cE = rd.point(pb), rd.point(pb)
        u0, X0 = case_inst(c)
        d = deferred(cid, Transcript(label), c["digest"], (cW, cE, u0 if u is None else u, X0 if X is None else list(X)), c["n_w"], c["n_c"], c["side_tag"], rd,
                     c["E"] is not None)
    except ValueError as e:
        return str(e)
    if isinstance(d, dict):
        d["trailing"] = rd.pos != len(rd.b)
    return d


# ---- the group side ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def key_limbs(cid):
    return np.array(to_limbs([co for pt in S.key_points(cid) for co in pt])).reshape(-1, 8)


def _lincomb(orc, cid, pts, scalars):
    acc = (0, 0)
    for Q, k in zip(pts, scalars):
        if tuple(Q) != (0, 0) and k:
            acc = orc.curve_add(cid, acc, orc.curve_mul(cid, Q, k))
    return acc


def _key_msm(orc, cid, acc):
    n = len(acc)
    return orc.msm(cid, key_limbs(cid)[:n], to_limbs(acc)) if any(acc) else (0, 0)


def opening_holds(orc, cid, op):
    """Σ c·Q + g·U == afin·<s, G> for one opening"""
    ps = S.FIELD[CURVE_SCALAR[cid]]
    return batch_holds(orc, cid, [op], [1], 1 << op["rounds"])[0]


def accumulators(ops, rhos, big, p):
    acc = [0] * big
    for op, rho in zip(ops, rhos):
        n, k = 1 << op["rounds"], rho * op["afin"] % p
        for i, si in enumerate(svec(op["xs"], p)):
            j = slot_of(i, n, op["shifted"])
            acc[j] = (acc[j] + k * si) % p
    return acc


def batch_holds(orc, cid, ops, rhos, big):
    """(the batch equation's verdict, the accumulators)"""
    ps = S.FIELD[CURVE_SCALAR[cid]]
    Ugen = ck_derive(cid, b"vimz-ipa-u", 0)
    lhs, gsum = (0, 0), 0
    for op, rho in zip(ops, rhos):
        bfin = masked_dot(op["xs"], op["pt"], op["n_pub"], op["n_w"], ps)
        gsum = (gsum + rho * (op["g0"] - op["afin"] * bfin * op["r0"])) % ps
        lhs = orc.curve_add(cid, lhs, _lincomb(orc, cid, op["Q"], [rho * ck % ps for ck in op["c"]]))
    lhs = orc.curve_add(cid, lhs, _lincomb(orc, cid, [Ugen], [gsum]))
    acc = accumulators(ops, rhos, big, ps)
    return tuple(lhs) == tuple(_key_msm(orc, cid, acc)), acc


def verify_bytes(orc, c, blob, label, u=None, X=None):
    """The deferred verifier end to end on one instance, every opening judged by its unrolled equation: None = accepted, else the failed check — the counterpart of
    _spartan_ref.verify_bytes / _spartan_pub_ref.verify_bytes."""
    d = deferred_bytes(c, blob, label, u, X)
    if isinstance(d, str):
        return d
    ps = S.FIELD[CURVE_SCALAR[c["cid"]]]
    if mat_eval(c, d["rx"], d["ry"], d["w"], ps) * d["vz"] % ps != d["claim"]:
        return "inner sum-check"
    for op, what in zip(d["openings"], ("opening of W", "opening of E")):
        if not opening_holds(orc, c["cid"], op):
            return what
    return "trailing bytes" if d["trailing"] else None


@functools.lru_cache(maxsize=None)
def proof_of(orc, name):
    """(case, label, bytes) of a named case of either module, proved once"""
    if name in P.case_names():
        c = P.case(name)
        return c, P.LABEL, P.prove(orc, c)[1]
    c = S.instance_case(name)
    return c, S.LABEL, S.prove_instance(orc, c)


def bump_final_scalar(c, blob, which="W"):
    """the blob with afin + 1 in its W (or E) opening"""
    ps = S.FIELD[CURVE_SCALAR[c["cid"]]]
    lay = S.argument_layout(c)
    off = 128 + lay["W opening's final scalar" if which == "W" else "E opening"]
    v = (int.from_bytes(blob[off:off + 32], "little") + 1) % ps
    return blob[:off] + v.to_bytes(32, "little") + blob[off + 32:]


# ---- cases of the kernel tests -------------------------------------------------------------------------------------------------------------------------------
SVEC_ROUNDS = tuple(sorted({1, 2, BLOCK_LOG2 - 1, BLOCK_LOG2, BLOCK_LOG2 + 1, SPLIT_H - 1, SPLIT_H, SPLIT_H + 1, 13}))      # (log2(block) + 1 is h − 1)
SVEC_GROUPS = (1, GROUP, GROUP + 1)
SVEC_BIG_ROUNDS = 19


def svec_case_names():
    return [f"{fid}/{rounds}/{n}" for fid in (0, 1) for rounds in SVEC_ROUNDS for n in SVEC_GROUPS]


def svec_case(name):
    """n openings of `rounds` challenges: shifted and unshifted mixed; masks at n_pub 1 and 7 with n_w = N (no padding) and N/2 + 1 (the most padding) where the
    shape allows; opening 0 has a challenge 0, the last a challenge r − 1."""
    fid, rounds, n = (int(x) for x in name.split("/"))
    p, N = S.FIELD[fid], 1 << rounds
    rng = S._rng("batch-svec", name)
    ops = []
    for o in range(n):
        xs = [rng.getrandbits(128) for _ in range(rounds)]
        if o == 0:
            xs[rounds // 2] = 0
        if o == n - 1:
            xs[0] = p - 1
        shifted = o % 2 == 0
        n_pub, n_w = 0, 0                          # an unshifted (E) opening has no mask
        if shifted:                                # over the rounds of SVEC_ROUNDS every pairing of n_pub in (1, 7) with n_w in (N, N/2 + 1) occurs
            n_pub = (1, 7)[(o // 2) % 2]
            n_w = (N, N // 2 + 1)[(o // 2 + rounds) % 2]
            if n_w < n_pub + 2:
                n_pub = 1
            if n_w < n_pub + 2:                    # (N = 2: no committed wire fits; no mask)
                n_pub, n_w = 0, 0
        ops.append({"xs": xs, "pt": [rng.randrange(p) for _ in range(rounds)], "coef": rng.randrange(p), "shifted": shifted, "n_pub": n_pub, "n_w": n_w})
    return {"fid": fid, "rounds": rounds, "ops": ops}


def svec_expected(case):
    """(acc over 2^rounds slots, [dot])"""
    p, n = S.FIELD[case["fid"]], 1 << case["rounds"]
    acc = [0] * n
    for op in case["ops"]:
        for i, si in enumerate(svec(op["xs"], p)):
            j = slot_of(i, n, op["shifted"])
            acc[j] = (acc[j] + op["coef"] * si) % p
    return acc, [masked_dot(op["xs"], op["pt"], op["n_pub"], op["n_w"], p) for op in case["ops"]]


def svec_big_case():
    """three openings at the workload's grid size: W, E, W"""
    rng = S._rng("batch-svec-big")
    p, N = S.FIELD[0], 1 << SVEC_BIG_ROUNDS
    ops = []
    for o in range(3):
        ops.append({"xs": [rng.getrandbits(128) for _ in range(SVEC_BIG_ROUNDS)], "pt": [rng.randrange(p) for _ in range(SVEC_BIG_ROUNDS)], "coef": rng.randrange(p),
                    "shifted": o != 1, "n_pub": 2 if o != 1 else 0, "n_w": N - 12345 if o != 1 else 0})
    return {"fid": 0, "rounds": SVEC_BIG_ROUNDS, "ops": ops}


def svec_big_expected(case):
    """the digests (S.table_digests) of the accumulator's bytes and the dots, by numpy-free integers over half-tables (the definition itself takes minutes at 2^19)"""
    p, rounds = S.FIELD[case["fid"]], case["rounds"]
    n, h = 1 << rounds, rounds // 2
    acc, dots = [0] * n, []
    for op in case["ops"]:
        xs, pt = op["xs"], op["pt"]
        s_hi, s_lo = svec(xs[:rounds - h], p), svec(xs[rounds - h:], p)
        b_hi, b_lo = S.eq_table(pt[:rounds - h], p), S.eq_table(pt[rounds - h:], p)
        dot, k, mask = 0, op["coef"], (1 << h) - 1
        for i in range(n):
            si = s_hi[i >> h] * s_lo[i & mask] % p
            j = slot_of(i, n, op["shifted"])
            acc[j] = (acc[j] + k * si) % p
            if not masked(i, op["n_pub"], op["n_w"]):
                dot += si * (b_hi[i >> h] * b_lo[i & mask] % p)
        dots.append(dot % p)
    raw = b"".join(v.to_bytes(32, "little") for v in acc)
    return S.table_digests(raw), dots


MAT_GROUPS = (1, GROUP, GROUP + 1)


def mat_shape_cases():
    """the relaxed instance shapes of _spartan_ref on both curves (4 x 2 … 513 x 512; the dense ones carry long and medium rows and repeated triplets)"""
    return [n for n in S.instance_names() if n.endswith("/relaxed")]


def mat_special_case(cid, kind):
    """a small shape with: an empty row, a medium row (7..32 terms), a long row (> 32 terms), a repeated triplet ("mixed"); or no entry in B at all ("empty")"""
    p = S.FIELD[CURVE_SCALAR[cid]]
    rng = S._rng("batch-mat", cid, kind)
    n_c, n_w = 9, 70
    nz = lambda: rng.randrange(1, p)      # noqa: E731
    out = {"cid": cid, "n_c": n_c, "n_w": n_w}
    for m in "ABC":
        rows = [[(rng.randrange(n_w), nz()) for _ in range(rng.randint(1, 4))] for _ in range(n_c)]
        rows[3] = []                                                       # an empty row
        rows[4] = [(c, nz()) for c in rng.sample(range(n_w), 12)]          # the medium class
        rows[5] = [(c, nz()) for c in rng.sample(range(n_w), 40)]          # the long class
        rows[6] = rows[6] + [rows[6][0], rows[6][0]]                       # repeated (row, column, value)
        out[m] = [(r, c, v) for r, terms in enumerate(rows) for c, v in terms]
        rng.shuffle(out[m])
    if kind == "empty":
        out["B"] = []
    return out


def mat_points(case, n, key):
    """n members' (rx, ry, w): member 0 has a coordinate 0 and one r − 1"""
    p = S.FIELD[CURVE_SCALAR[case["cid"]]]
    s, t = (case["n_c"] - 1).bit_length(), (case["n_w"] - 1).bit_length()
    rng = S._rng("batch-mat-points", key, n)
    out = []
    for g in range(n):
        rx, ry = [rng.randrange(p) for _ in range(s)], [rng.randrange(p) for _ in range(t)]
        if g == 0:
            rx[0], ry[-1] = 0, p - 1
        rho = rng.getrandbits(128)
        out.append((rx, ry, (1, rho, rho * rho % p)))
    return out
