"""Integer reference and case tables for the stage tests of the MSM's head (vimz_amd/csrc/msm.hpp): the digit producers (load_scalar, for_each_digit,
signed_digit<7>), both counting sorts (k_hist_lds / k_scatter_lds, k_hist / k_scatter with agg_atomic_inc), k_accum, the unit sums (k_ones_partial, k_ones_dense,
k_ones_dense_rows), the fused paths (k_msm_small with its ticket merge or k_msm_small_sum, k_msm_fixed) and the table builders (k_build_tables,
k_build_multiples).  Test infrastructure.

Plain Python integers only.  The curve arithmetic, the point pool and the slot decoding are those of tests/_msm_tail_ref.py; `digits` and `boundary_values` those
of tests/_signed_scalars.py (tests/test_msm_head_ref_host.py checks this module against both and against the oracle's MSM).  Bases are known multiples k_i·G
— repeated k, negated k and the identity (k = 0) among them — so that what a kernel must produce is (a sum of integers)·G, compared exactly."""
import random

import numpy as np

from tests import _msm_tail_ref as T
from tests._signed_scalars import boundary_values, digits  # noqa: F401 — `digits` is what signed_digits is checked against

CURVES, CURVE_NAMES = T.CURVES, T.CURVE_NAMES
FIELDS = (0, 1, 2, 3)                                   # VIMZ_FIELD_BN254_FR, _FQ, _PALLAS_FP, _VESTA_FQ
FIELD_P = T.MODULUS
SCALAR_FIELD = (0, 1, 3, 2)                             # curve -> the field of its scalars
R256 = 1 << 256                                         # Montgomery radix of the 8 x 32-bit scalar fields
FORMS = (0, 1)                                          # VIMZ_FORM_CANONICAL, VIMZ_FORM_MONTGOMERY
SMALL_C, SMALL_NBW, SMALL_CHUNK, SMALL_MAXQ, SMALL_THREADS = 7, 64, 1536, 32, 256      # msm_shape.hpp / msm.hpp
FIXED_CHUNK = 1024
ONES_THREADS = 16384
TOTALS_WORDS = 16
UNWRITTEN = 0xffffffff


def windows(p, c):
    """K of a plan: ceil((bits of p + 1) / c)"""
    return (p.bit_length() + c) // c


def to_form(s, p, form):
    """the 256-bit word a scalar travels as"""
    return s * R256 % p if form else s


def words_u64(vals):
    """integers below 2^256 -> (n, 4) uint64"""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (v >> (64 * k)) & 0xffffffffffffffff
    return out


# ---- the digit producers ------------------------------------------------------------------------------------------------------------------------
def load_scalar(word, p, form, skip_ones, sgn):
    """msm.hpp's load_scalar on the 256-bit word as it lies in memory: None (skipped), or (s, flip)"""
    if word == 0:
        return None
    if skip_ones and word == (R256 % p if form else 1):
        return None
    s = word * pow(R256, -1, p) % p if form else word
    if sgn and s <= p and p - s < s:
        return p - s, 1
    return s, 0


def signed_digits(s, c, K):
    """for_each_digit: the K signed digits of s in [-(2^(c-1) - 1), 2^(c-1)], low window first (bits past 256 read as zero)"""
    half, carry, out = 1 << (c - 1), 0, []
    s &= R256 - 1
    for w in range(K):
        d = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        carry = 1 if d > half else 0
        out.append(d - (1 << c) if carry else d)
    return out


_T7 = [sum(64 << (SMALL_C * j) for j in range(w)) for w in range(40)]


def signed_digit7(s, w):
    """signed_digit<7>: digit w WITHOUT the walk — the carry into window w is one exactly when the low 7w bits exceed T_w = sum_{j<w} 64·128^j"""
    lo = SMALL_C * w
    t = _T7[w]
    carry = 1 if (s & ((1 << lo) - 1)) > t else 0
    d = ((s >> lo) & 127) + carry
    return d - 128 if d > 64 else d


def scalar_digits7(word, p, form, sgn, K):
    """the K digits the fused kernels take of a scalar's word (all zero for a skipped one)"""
    ls = load_scalar(word, p, form, 0, sgn)
    if ls is None:
        return [0] * K
    s, flip = ls
    return [-signed_digit7(s, w) if flip else signed_digit7(s, w) for w in range(K)]


def small_sub_len(counts):
    """k_msm_small's sub-bucket length for a chunk's 64 bucket counts: the shortest of 4..8 whose sub-buckets still get one of 256 threads each"""
    for sub in (4, 5, 6, 7):
        if sum((n + sub - 1) // sub for n in counts) <= SMALL_THREADS:
            return sub
    return 8


def chunk_bucket_counts(ds):
    """bucket counts (64) of one chunk's digits of one window"""
    cnt = [0] * SMALL_NBW
    for d in ds:
        if d:
            cnt[abs(d) - 1] += 1
    return cnt


# ---- scalars --------------------------------------------------------------------------------------------------------------------------------------
def near_units(p, form):
    """words that are NOT the unit but share all words but one with it: 1 with one other word set; the Montgomery unit with one word changed"""
    r1 = R256 % p
    if form:
        out = [r1 ^ (1 << (32 * k)) for k in range(8)]
        return [w for w in out if 0 < w < R256]
    return [1 | (1 << (32 * k)) for k in range(1, 8) if (1 | (1 << (32 * k))) < p]


def edge_scalars(p, c):
    """the scalars every digit case holds (canonical integers): the boundary values, (p - 1)/2 next to (p + 1)/2, a digit of exactly 2^(c-1) (stays positive) and
    2^(c-1) + 1 (negative, with a carry) in the bottom and in an upper window, 2^k - 1 for every k (a carry through every window), p - 1"""
    half = 1 << (c - 1)
    out = list(boundary_values(p)) + [(p - 1) // 2, (p + 1) // 2, half, half + 1, half << c, (half + 1) << c, (half << (3 * c)) | half, ((half + 1) << (3 * c)) | (half + 1)]
    out += [(1 << k) - 1 for k in range(1, p.bit_length())] + [p - 1]
    return out


def scalar_words(field, n, c, form, kind="edges"):
    """n words of a digit case: the edge scalars (the first ones of every vector, as many as fit; with the near-units of the form after every 37th),
    then seeded random ones, dense and short, of both signs"""
    p = FIELD_P[field]
    if kind == "all_zero":
        return [0] * n
    if kind == "all_one":
        return [to_form(1, p, form)] * n
    rng = random.Random(f"msm-head/scalars/{field}/{n}/{c}")
    edges, nu = edge_scalars(p, c), near_units(p, form)
    rng.shuffle(edges)
    edges = [p - 1, 1, 0, (p - 1) // 2, (p + 1) // 2, 1 << (c - 1), (1 << (c - 1)) + 1] + edges
    out, e = [], 0
    for i in range(n):
        if i % 37 == 5:
            out.append(nu[(i // 37) % len(nu)])
        elif e < len(edges):
            out.append(to_form(edges[e], p, form))
            e += 1
        else:
            k = rng.random()
            s = rng.randrange(p) if k < 0.5 else rng.getrandbits(70) if k < 0.7 else p - 1 - rng.getrandbits(70) if k < 0.9 else rng.choice(edges)
            out.append(to_form(s, p, form))
    return out


# ---- sort -----------------------------------------------------------------------------------------------------------------------------------------
SORT_C_LDS = ((2, 0), (5, 0), (7, 0), (11, 0), (15, 1), (16, 1))      # (c, shared bucket set) through k_hist_lds / k_prefix_scan / k_scatter_lds
SORT_C_GLOBAL = ((7, 0), (12, 0), (16, 1))                            # through k_hist / k_scan / k_scatter (agg_atomic_inc)
SORT_N = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
SORT_BLOCKS = (1, 2, 32, 256)
SORT_SUB, SORT_HEAVY_MIN = (8, 16), 32
AGG_DISTINCT = (1, 2, 3, 5, 16, 64)                                   # distinct values in every run of 64 consecutive scalars
AGG_N = 4 * 64 + 29                                                   # four full waves and a short one
LDS_LIMIT = 144 * 1024


def sort_pstride(n, shared):
    return n + 3 if shared else 0                                     # a table row longer than the vector


def agg_words(field, distinct, zeros, c, form):
    """AGG_N words whose every aligned run of 64 holds `distinct` distinct non-zero values (small ones: one digit each, in window 0, so a wave's lanes meet in
    `distinct` counters) — zeros != 0: every third scalar is zero instead (inactive lanes between the groups; 43 lanes are then left for the values).  Group j of a
    run takes about half the lanes of group j - 1, and the groups lie in descending size from a start that moves with the run: groups of four lanes and more (a
    leader round each), a group of fewer than four (the early break) and lanes left after four rounds (the per-lane fallback) all occur."""
    p = FIELD_P[field]
    assert distinct <= 1 << (c - 1)
    out = []
    for i in range(AGG_N):
        lane, run = i % 64, i // 64
        active = [x for x in range(64) if not (zeros and x % 3 == 2)]
        if lane not in active:
            out.append(0)
            continue
        D = min(distinct, len(active))
        sizes, rem = [1] * D, len(active) - D
        for j in range(D):
            add = min(rem, max(0, (64 >> (j + 1)) - 1))
            sizes[j] += add
            rem -= add
        sizes[0] += rem
        order = [j for j in range(D) for _ in range(sizes[j])]
        order = order[-(run * 5) % len(order):] + order[:-(run * 5) % len(order)] if run else order
        out.append(to_form(1 + order[active.index(lane)], p, form))
    return out


def agg_pattern(words):
    """how agg_atomic_inc serves the first full wave of a vector of one-digit scalars: (leader rounds run, lanes served by the per-lane fallback, whether the
    loop ended on the early break) — the model the host test holds the agg cases against"""
    lanes = [w for w in words[:64]]
    pending = [i for i, w in enumerate(lanes) if w]
    rounds, early = 0, False
    for _ in range(4):
        if not pending:
            break
        lead = lanes[pending[0]]
        same = [i for i in pending if lanes[i] == lead]
        pending = [i for i in pending if lanes[i] != lead]
        rounds += 1
        if len(same) < 4:
            early = True
            break
    return rounds, len(pending), early


def sort_cases():
    """name -> dict(field, form, sgn, skip_ones, c, shared, lds, n, sort_blocks, sub, kind).  The grid (c, layout, lds) x n runs over rotating fields, forms, sgn,
    skip_ones and sort_blocks; every one of the 32 (field, form, sgn, skip_ones) combinations runs at one small shape through both sorts; then the vectors of one
    value (all zero, all one under both skip_ones) and the agg_atomic_inc patterns."""
    cases, j = {}, 0
    for lds, table in ((1, SORT_C_LDS), (0, SORT_C_GLOBAL)):
        for c, shared in table:
            for n in SORT_N:
                cases[f"grid/lds={lds}/c={c}/n={n}"] = dict(field=j % 4, form=(j // 4) % 2, sgn=(j // 8 + j) % 2, skip_ones=(j // 16 + j // 2) % 2, c=c, shared=shared, lds=lds,
                                                          n=n, sort_blocks=SORT_BLOCKS[(j + j // 4) % 4], sub=SORT_SUB[j % 2], kind="edges")
                j += 1
    for field in FIELDS:
        for form in FORMS:
            for sgn in (0, 1):
                for skip in (0, 1):
                    for lds in (1, 0):
                        cases[f"combo/field={field}/form={form}/sgn={sgn}/skip_ones={skip}/lds={lds}"] = dict(
                            field=field, form=form, sgn=sgn, skip_ones=skip, c=7, shared=0, lds=lds, n=321, sort_blocks=2, sub=8, kind="edges")
    for field in FIELDS:
        for form in FORMS:
            for lds in (1, 0):
                cases[f"all_zero/field={field}/form={form}/lds={lds}"] = dict(field=field, form=form, sgn=1, skip_ones=0, c=7, shared=0, lds=lds, n=65, sort_blocks=2, sub=8,
                                                                             kind="all_zero")
                for skip in (0, 1):
                    cases[f"all_one/field={field}/form={form}/skip_ones={skip}/lds={lds}"] = dict(field=field, form=form, sgn=1, skip_ones=skip, c=7, shared=0, lds=lds,
                                                                                                   n=65, sort_blocks=32, sub=8, kind="all_one")
    for i, distinct in enumerate(AGG_DISTINCT):
        for zeros in (0, 1):
            c, shared = SORT_C_GLOBAL[(i + zeros) % 3]
            cases[f"agg/distinct={distinct}/zeros={zeros}"] = dict(field=(i + zeros) % 4, form=i % 2, sgn=zeros, skip_ones=0, c=c, shared=shared, lds=0, n=AGG_N, sort_blocks=1,
                                                                   sub=8, kind=("agg", distinct, zeros))
    # the block counts that leave workgroups an empty chunk (n < sort_blocks) and a short last chunk, named
    cases["blocks/n=65/sort_blocks=256"] = dict(field=0, form=0, sgn=1, skip_ones=1, c=11, shared=0, lds=1, n=65, sort_blocks=256, sub=16, kind="edges")
    cases["blocks/n=1/sort_blocks=32"] = dict(field=1, form=1, sgn=1, skip_ones=0, c=5, shared=0, lds=1, n=1, sort_blocks=32, sub=8, kind="edges")
    cases["blocks/n=1025/sort_blocks=32"] = dict(field=2, form=0, sgn=0, skip_ones=1, c=15, shared=1, lds=1, n=1025, sort_blocks=32, sub=16, kind="edges")
    return cases


def sort_words(case):
    if isinstance(case["kind"], tuple):
        return agg_words(case["field"], case["kind"][1], case["kind"][2], case["c"], case["form"])
    return scalar_words(case["field"], case["n"], case["c"], case["form"], case["kind"])


def sort_shape(case):
    """(K, nbw, nb, bstride, pstride) of a sort case"""
    K = windows(FIELD_P[case["field"]], case["c"])
    nbw = 1 << (case["c"] - 1)
    return K, nbw, (nbw if case["shared"] else nbw * K), (0 if case["shared"] else nbw), sort_pstride(case["n"], case["shared"])


def sort_ref(words, p, form, skip_ones, sgn, c, K, bstride, pstride, nb, sub):
    """(counts, bucket_off, sub_off, totals[4], entries as (bucket, value) pairs) — value = (index + window·pstride) | negative << 31"""
    ent = []
    for i, word in enumerate(words):
        ls = load_scalar(word, p, form, skip_ones, sgn)
        if ls is None:
            continue
        s, flip = ls
        for w, d in enumerate(signed_digits(s, c, K)):
            if d:
                ent.append((w * bstride + abs(d) - 1, (i + w * pstride) | (((1 if d < 0 else 0) ^ flip) << 31)))
    counts = np.zeros(nb, dtype=np.uint64)
    if ent:
        np.add.at(counts, np.array([g for g, _ in ent]), 1)
    boff = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    soff = np.concatenate([[0], np.cumsum((counts + sub - 1) // sub)]).astype(np.uint64)
    return counts, boff, soff, [int(soff[-1]), int(boff[-1]), 0, 0], ent


# ---- accumulate -----------------------------------------------------------------------------------------------------------------------------------
# The key of the accumulate cases: index 0 the identity, 1..40 distinct points, 41 the same point as 5, 42 the negative of 6.
ACCUM_KEY = [0] + list(range(1, 41)) + [5, -6]
ACCUM_SUB = (8, 16)
ACCUM_TOTALS = (0, 1, 255, 256, 257)
ACCUM_ROWS = (1, 3, 16)
# pieces planted inside one sub-bucket: (index, negative) in order
ACCUM_PLANTED = {
    "doubling_first": [(5, 0), (5, 0)],
    "doubling_mid_chain": [(3, 0), (4, 0), (7, 0), (9, 0)],                     # 3 + 4 = 7: the third addition doubles
    "same_point_other_index": [(5, 0), (41, 0), (2, 0)],
    "cancel_then_more": [(5, 0), (5, 1), (8, 0)],                               # P, -P, Q: through the identity
    "cancel_mid_chain": [(3, 0), (4, 0), (7, 1), (9, 0)],
    "negated_base_cancels": [(6, 0), (42, 0)],                                  # ends on the identity
    "identity_first": [(0, 0), (3, 0), (4, 0)], "identity_first_signed": [(0, 1), (3, 0), (4, 0)],
    "identity_middle": [(3, 0), (0, 0), (4, 0)], "identity_middle_signed": [(3, 1), (0, 1), (4, 0)],
    "identity_last": [(3, 0), (4, 0), (0, 0)], "identity_last_signed": [(3, 0), (4, 1), (0, 1)],
    "identity_alone_signed": [(0, 1)],
}


def accum_layout(sub, total, row=0):
    """the buckets of one row, as lists of (index, negative): runs of empty buckets at the start, in the middle and at the end; buckets of sub - 1, sub, sub + 1 and
    2·sub entries; the planted pieces; then buckets of one or two entries until the row holds exactly `total` sub-buckets (total = 0: every bucket empty; 1: one entry)"""
    rng = random.Random(f"msm-head/accum/{sub}/{total}/{row}")
    gen = lambda m: [(rng.randrange(1, 41), rng.randrange(2)) for _ in range(m)]      # noqa: E731
    empty = [[] for _ in range(5 + row % 3)]
    if total == 0:
        return empty + empty
    if total == 1:
        return empty + [[(7, 1)]] + empty
    buckets = list(empty)
    sized = [gen(m) for m in (sub - 1, sub, sub + 1, 2 * sub)]
    planted = [list(v) for v in ACCUM_PLANTED.values()]
    planted = planted[row % len(planted):] + planted[:row % len(planted)]
    buckets += sized[:2] + [[] for _ in range(67)] + sized[2:] + planted[:6] + [[]] + planted[6:]
    # a planted piece that shares a bucket with a full piece before it: the piece starts exactly at a multiple of sub
    buckets.append(gen(sub) + list(ACCUM_PLANTED["doubling_mid_chain"]))
    subs = sum((len(b) + sub - 1) // sub for b in buckets)
    assert subs <= total, (subs, total)
    while subs < total:
        buckets.append(gen(1 + (subs + row) % 2))
        subs += 1
        if subs % 9 == 0:
            buckets.append([])
    return buckets + [[] for _ in range(3 + row % 2)]


def accum_arrays(sub, total, rows):
    """(sorted rows x entries, bucket_off, sub_off rows x (nb + 1), totals rows x 16, layouts) of a case; entries = the longest row's + 5 unwritten words"""
    layouts = [accum_layout(sub, total, r) for r in range(rows)]
    nb = max(len(b) for b in layouts)
    layouts = [b + [[] for _ in range(nb - len(b))] for b in layouts]
    entries = max(sum(len(x) for x in b) for b in layouts) + 5
    srt = np.full((rows, entries), UNWRITTEN, dtype=np.uint32)
    boff, soff = np.zeros((rows, nb + 1), dtype=np.uint32), np.zeros((rows, nb + 1), dtype=np.uint32)
    totals = np.zeros((rows, TOTALS_WORDS), dtype=np.uint32)
    for r, b in enumerate(layouts):
        flat = [i | (s << 31) for x in b for i, s in x]
        srt[r, :len(flat)] = flat
        boff[r, 1:] = np.cumsum([len(x) for x in b])
        soff[r, 1:] = np.cumsum([(len(x) + sub - 1) // sub for x in b])
        totals[r, 0], totals[r, 1] = soff[r, nb], boff[r, nb]
        assert totals[r, 0] == total
    return srt, boff, soff, totals, layouts


def accum_ref(layout, sub):
    """the scalar of every sub-bucket's partial, in slot order"""
    out = []
    for b in layout:
        for k in range(0, len(b), sub):
            out.append(sum(-ACCUM_KEY[i] if s else ACCUM_KEY[i] for i, s in b[k:k + sub]))
    return out


ACCUM_CASES = [(sub, total, rows) for sub in ACCUM_SUB for total in ACCUM_TOTALS for rows in ACCUM_ROWS if rows == 1 or total >= 255]


# ---- keys of the fused cases ------------------------------------------------------------------------------------------------------------------------
def key_ks(n, kind="mixed"):
    """the multiples k_i of G a key of n points holds: distinct small ones with a repeated k, a negated k and the identity planted among them"""
    if kind == "all_equal":
        return [9] * n
    ks = [1 + (i * 7) % 4093 for i in range(n)]
    for i in range(n):
        if i % 11 == 3:
            ks[i] = 0
        elif i % 11 == 7:
            ks[i] = -ks[i - 1]
        elif i % 13 == 5:
            ks[i] = ks[i - 1]
    return ks


def key_points(c, ks):
    """(n, 8) uint64 canonical affine points, the identity as zeros"""
    pts = []
    for k in ks:
        x, y = T.mul(c, k) if k else (0, 0)
        pts += [x, y]
    return words_u64(pts).reshape(len(ks), 8)


# ---- fused small ------------------------------------------------------------------------------------------------------------------------------------
SMALL_N_Q1 = (1, 255, 256, 257, 1536)
SMALL_Q_CHUNK3 = (2, 3, 4, 5, 7, 8, 20)
SMALL_TAILS = (0, 1)                                    # 0: the ticket merge inside k_msm_small; 1: k_msm_small_sum
SMALL_BIG_CURVE = 0                                     # Q = 20 at chunk = 1536
SUBLEN_DISTRIBUTIONS = {                                # bucket counts of a chunk's window 0 for which the model picks each length
    4: [16] * 64, 5: [17] * 64, 6: [24] * 64, 7: [19] * 63 + [25], 8: [22] * 63 + [29],
}
CRAFTED = ("one_value_1536", "one_per_bucket", "bucket_63_alone", "sublen_4", "sublen_5", "sublen_6", "sublen_7", "sublen_8", "identity_under_negative_digit", "all_bases_equal",
           "p_next_to_minus_p")


def digit0_scalar(d):
    """the smallest non-negative scalar whose window-0 digit (c = 7) is d"""
    return d if d > 0 else 128 + d


def crafted(kind):
    """(canonical scalars, key ks) of a crafted case of the fused small path — one chunk"""
    if kind == "one_value_1536":                        # one bucket of 1536 entries: 256 sub-buckets of 6, a segmented tree of depth 8
        return [5] * 1536, key_ks(1536)
    if kind == "one_per_bucket":
        return [digit0_scalar(d) for d in range(1, 65)], key_ks(64)
    if kind == "bucket_63_alone":
        return [64], [3]
    if kind.startswith("sublen_"):
        counts = SUBLEN_DISTRIBUTIONS[int(kind[-1])]
        sc = [digit0_scalar((b + 1) if (b + j) % 3 else -(b + 1) if b < 63 else 64) for b, m in enumerate(counts) for j in range(m)]
        random.Random(kind).shuffle(sc)
        return sc, key_ks(len(sc))
    if kind == "identity_under_negative_digit":         # every base the identity or next to it, every window-0 digit negative
        sc = [digit0_scalar(-(1 + i % 5)) for i in range(40)]
        return sc, [0 if i % 2 == 0 else 4 for i in range(40)]
    if kind == "all_bases_equal":
        return [digit0_scalar((1 + i % 9) * (-1 if i % 4 == 1 else 1)) for i in range(300)], key_ks(300, "all_equal")
    if kind == "p_next_to_minus_p":                     # P and -P (a negated base) with the same digit: one bucket, neighbours in its list; and P under d next to P under -d
        ks = [6, -6, 8, 8, 11, -11, 11]
        return [digit0_scalar(d) for d in (7, 7, 9, -9, 64, 64, 64)], ks
    raise ValueError(kind)


def small_cases():
    """name -> dict(curve, form, sgn, tail, calls, n, Q, chunk, tables, offset, kind).  Every shape on all four curves with form, sgn, tail and calls rotating over the
    shapes; every one of the 16 (form, sgn, tail, calls) combinations at Q = 3 on every curve; the crafted chunks on all four curves; tables with a base offset."""
    cases, j = {}, 0
    for c in CURVES:
        shapes = [(n, 1, n, "edges") for n in SMALL_N_Q1] + [(1537, 2, 769, "edges")] + [(3 * Q - 1, Q, 3, "edges") for Q in SMALL_Q_CHUNK3]
        if c == SMALL_BIG_CURVE:
            shapes.append((20 * 1536, 20, 1536, "edges"))
        for n, Q, chunk, kind in shapes:
            for tables in (0, 1):
                if tables and (n > 1537 or (Q not in (1, 2, 5) and c)):
                    continue
                cases[f"shape/{CURVE_NAMES[c]}/n={n}/Q={Q}/chunk={chunk}/tables={tables}"] = dict(
                    curve=c, form=j % 2, sgn=(j // 2 + j // 8) % 2, tail=(j // 4 + j) % 2 if Q > 1 else 0, calls=1 + (j // 3) % 2, n=n, Q=Q, chunk=chunk, tables=tables,
                    offset=(5 if tables else 0), kind=kind)
                j += 1
        for form in FORMS:
            for sgn in (0, 1):
                for tail in SMALL_TAILS:
                    for calls in (1, 2):
                        cases[f"combo/{CURVE_NAMES[c]}/form={form}/sgn={sgn}/tail={tail}/calls={calls}"] = dict(
                            curve=c, form=form, sgn=sgn, tail=tail, calls=calls, n=8, Q=3, chunk=3, tables=0, offset=0, kind="edges")
        for i, kind in enumerate(CRAFTED):
            cases[f"crafted/{CURVE_NAMES[c]}/{kind}"] = dict(curve=c, form=(i + c) % 2, sgn=(i // 2) % 2, tail=0, calls=1, n=None, Q=1, chunk=None, tables=(i + c) % 4 == 3,
                                                             offset=(2 if (i + c) % 4 == 3 else 0), kind=kind)
    return cases


def fused_inputs(case):
    """(words, ks of the n points the scalars meet) of a small or fixed case"""
    c = case["curve"]
    p = FIELD_P[SCALAR_FIELD[c]]
    if case["kind"] == "edges":
        return scalar_words(SCALAR_FIELD[c], case["n"], SMALL_C, case["form"]), key_ks(case["n"])
    sc, ks = crafted(case["kind"])
    return [to_form(s, p, case["form"]) for s in sc], ks


def window_sums_ref(c, words, ks, form, sgn, tables):
    """the K integers a fused kernel's window sums must be multiples of G by: sum_i d_(i,w)·k_i, with tables times 2^(7w); mod the group order"""
    p = FIELD_P[SCALAR_FIELD[c]]
    K = windows(p, SMALL_C)
    acc = [0] * K
    for word, k in zip(words, ks):
        if k:
            for w, d in enumerate(scalar_digits7(word, p, form, sgn, K)):
                acc[w] += d * k
    return [(a << (SMALL_C * w) if tables else a) % T.ORDER[c] for w, a in enumerate(acc)]


def msm_scalar(c, words, ks, form):
    """sum s_i·k_i mod the group order: what the window sums of any path must fold to"""
    p = FIELD_P[SCALAR_FIELD[c]]
    ri = pow(R256, -1, p)
    return sum((w * ri % p if form else w) * k for w, k in zip(words, ks)) % T.ORDER[c]


def fold_window_sums(c, sums, tables):
    """window-sum scalars -> the MSM's scalar: added (tables), or by Horner over windows of 7 bits"""
    if tables:
        return sum(sums) % T.ORDER[c]
    acc = 0
    for s in reversed(sums):
        acc = (acc << SMALL_C) + s
    return acc % T.ORDER[c]


def chunk_sublens(case):
    """{(window, chunk): sub-bucket length the model picks} of a small case"""
    c = case["curve"]
    p = FIELD_P[SCALAR_FIELD[c]]
    K = windows(p, SMALL_C)
    words, _ = fused_inputs(case)
    n = len(words)
    Q, chunk = (case["Q"], case["chunk"]) if case["n"] is not None else (1, n)
    dig = [scalar_digits7(w, p, case["form"], case["sgn"], K) for w in words]
    return {(w, q): small_sub_len(chunk_bucket_counts([d[w] for d in dig[q * chunk:(q + 1) * chunk]])) for w in range(K) for q in range(Q)}


# ---- fixed-base and the tables ------------------------------------------------------------------------------------------------------------------------
FIXED_N = (1, 255, 256, 257, 1024, 1025)
FIXED_BIG_CURVE, FIXED_BIG_N = 0, (2049, 4097)
TABLE_C = (7, 11, 15)
TABLE_N = (1, 255, 256, 257)
TABLE_M = (1, 2, 63, 64)


def fixed_cases():
    cases, j = {}, 0
    for c in CURVES:
        for n in FIXED_N + (FIXED_BIG_N if c == FIXED_BIG_CURVE else ()):
            for calls in (1, 2):
                cases[f"{CURVE_NAMES[c]}/n={n}/calls={calls}"] = dict(curve=c, form=j % 2, sgn=(j // 2) % 2, calls=calls, n=n, offset=0, kind="edges")
                j += 1
        cases[f"{CURVE_NAMES[c]}/base_offset"] = dict(curve=c, form=c % 2, sgn=1, calls=2, n=250, offset=7, kind="edges")
    return cases


def table_cases():
    """(curve, c, n): the key of n points (index n // 2 the identity when n > 2) and the entries read of its tables"""
    return [(c, tc, n) for c in CURVES for tc in TABLE_C for n in TABLE_N]


def table_key(n):
    ks = key_ks(n)
    ks[0] = 2
    ks[n - 1] = 4091 if n > 1 else 2
    if n > 2:
        ks[n // 2] = 0
    return ks


def table_entries(c, tc, n):
    """[(which, w, i, m, scalar)]: which = 0 a window table's row w, point i (2^(tc·w)·k_i); 1 the multiples' (w, i, m) (m·2^(7w)·k_i; tc = 7 only)"""
    K = windows(FIELD_P[SCALAR_FIELD[c]], tc)
    ks = table_key(n)
    pts = sorted({0, n // 2, n - 1})
    out = [(0, w, i, 0, (ks[i] << (tc * w)) % T.ORDER[c]) for w in (0, 1, K - 1) for i in pts]
    if tc == SMALL_C:
        out += [(1, w, i, m, (m * ks[i] << (tc * w)) % T.ORDER[c]) for w in (0, 1, K - 1) for i in pts for m in TABLE_M]
    return out


# ---- unit sums ----------------------------------------------------------------------------------------------------------------------------------------
ONES_N = (1, 63, 64, 65, 128, 129)
ONES_BIG_N = 3 * ONES_THREADS + 64
ONES_KINDS = (0, 1, 2)                                  # k_ones_partial, k_ones_dense (each with its tree), k_ones_dense_rows + k_tree_rows
ONES_ROWS = (1, 2, 32)
# units among the 64 scalars a wave reads in each of its passes — the fill of its queue after the passes: 63 + 1 reaches 64 exactly; 63 + 64 crosses it and peaks at
# 127; 64 + 0 + 1 drains a full queue and starts again; 0 + 0 + 1 fills late.  Wave w of the first workgroup takes pattern w; wave 0 has a fourth, short pass.
ONES_QUEUE_PATTERNS = ((63, 1, 0), (63, 64, 0), (64, 0, 1), (0, 0, 1))
ONES_CONTENT = ("mixed", "no_units", "all_units", "near_units")


def ones_words(c, n, form, content, row=0):
    """n words of a unit-sum case"""
    p = FIELD_P[SCALAR_FIELD[c]]
    one, nu = to_form(1, p, form), near_units(p, form)
    rng = random.Random(f"msm-head/ones/{c}/{n}/{content}/{row}")
    if content == "all_units":
        return [one] * n
    if content == "near_units":                         # no unit at all: every word differs from it in one word
        return [nu[(i + row) % len(nu)] for i in range(n)]
    if content == "no_units":
        return [to_form(2 + rng.randrange(p - 2), p, form) if i % 3 else 0 for i in range(n)]
    if content == "queue":
        out = [to_form(2 + rng.randrange(1 << 60), p, form) for _ in range(n)]
        for wave, pat in enumerate(ONES_QUEUE_PATTERNS):
            for ps, units in enumerate(pat):
                base = ps * ONES_THREADS + 64 * wave
                lanes = list(range(64))
                rng.shuffle(lanes)
                for lane in lanes[:units]:
                    out[base + lane] = one
        out[3 * ONES_THREADS + 5] = out[3 * ONES_THREADS + 63] = one         # wave 0's short fourth pass
        out[ONES_THREADS - 1] = out[2 * ONES_THREADS - 64] = one             # the last wave's passes
        return out
    return [one if rng.random() < 0.45 else nu[i % len(nu)] if i % 7 == 0 else 0 if i % 5 == 0 else to_form(rng.randrange(p), p, form) for i in range(n)]


def ones_ref(words, ks, p, form):
    one = to_form(1, p, form)
    return sum(k for w, k in zip(words, ks) if w == one)


def queue_fills(words, p, form, wave):
    """the fill of wave `wave`'s queue after each of its passes, before the drain (k_ones_dense: ones_dense_sum)"""
    one, cnt, out = to_form(1, p, form), 0, []
    for base in range(64 * wave, len(words), ONES_THREADS):
        cnt += sum(1 for w in words[base:base + 64] if w == one)
        out.append(cnt)
        if cnt >= 64:
            cnt -= 64
    return out


def ones_cases():
    """name -> dict(curve, form, kind, rows, n, content)"""
    cases, j = {}, 0
    for c in CURVES:
        for form in FORMS:
            for n in ONES_N:
                for kind in ONES_KINDS:
                    rows = ONES_ROWS[(j // 3) % 3] if kind == 2 else 1
                    cases[f"{CURVE_NAMES[c]}/form={form}/n={n}/kind={kind}"] = dict(curve=c, form=form, kind=kind, rows=rows, n=n, content=ONES_CONTENT[j % 4] if n > 1 else "all_units")
                    j += 1
            for kind in ONES_KINDS:
                cases[f"{CURVE_NAMES[c]}/form={form}/queue/kind={kind}"] = dict(curve=c, form=form, kind=kind, rows=1, n=ONES_BIG_N, content="queue")
                cases[f"{CURVE_NAMES[c]}/form={form}/no_units/kind={kind}"] = dict(curve=c, form=form, kind=kind, rows=2 if kind == 2 else 1, n=129, content="no_units")
                cases[f"{CURVE_NAMES[c]}/form={form}/near_units/kind={kind}"] = dict(curve=c, form=form, kind=kind, rows=32 if kind == 2 else 1, n=65, content="near_units")
    return cases


# ---- invalid layouts: one refusal per validation rule of the hooks ---------------------------------------------------------------------------------------
INVALID = ("sort_lds_counters_past_144_KiB", "sort_c_outside_2_16", "sort_blocks_outside_1_256", "sort_sorted_too_short", "accum_offsets_not_monotone",
           "accum_sub_off_inconsistent", "accum_index_outside_the_key", "accum_rows_above_16", "small_n_outside_the_chunks", "small_chunk_above_1536", "small_Q_above_32",
           "small_tables_missing", "fixed_tables_missing", "ones_rows_above_32", "ones_n_outside_the_key", "tables_entry_outside")


# ---- the groups of the GPU test (tests/_msm_head_gpu.py runs every case of a group and prints how many it ran) -----------------------------------------------
GROUPS = ("sort", "accum", "small", "fixed", "tables", "ones", "invalid")


def group_cases(group):
    if group == "sort":
        return list(sort_cases())
    if group == "accum":
        return [(c, sub, total, rows) for c in CURVES for sub, total, rows in ACCUM_CASES]
    if group == "small":
        return list(small_cases())
    if group == "fixed":
        return list(fixed_cases())
    if group == "tables":
        return table_cases()
    if group == "ones":
        return list(ones_cases())
    if group == "invalid":
        return list(INVALID)
    raise ValueError(group)
