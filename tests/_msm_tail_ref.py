"""Integer reference and case tables for the stage tests of the large MSM's tail (vimz_amd/csrc/msm.hpp: k_scan / k_prefix_scan, k_combine, k_reduce,
k_reduce_planes, k_tree256, k_tree_rows) and of the four-lane additions under them (ec_mem.hpp: quad_level, quad_tree256).  Test infrastructure.

Plain Python integers only: nothing here comes from oracle/ or from the library (tests/test_msm_tail_ref_host.py checks this module against the oracle).
A point travels as a raw XYZZ slot in the resident layout of store_xyzz / load_xyzz: 40 words, X, Y, ZZ, ZZZ of nine 29-bit limbs in ten words each,
Montgomery radix 2^261 (tests/_fp29_ref.py), x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2, the identity ZZ = 0 (all words zero).  Any representative inside the
bounds of ec.hpp is a valid slot: X < 5.3 p, Y < 3.4 p, ZZ and ZZZ < 1.5 p.

Points are known multiples k·G, so that the sum a kernel must produce is (sum of the k)·G: a `spec` is (k, z, (lx, ly, lzz, lzzz)) — the point k·G (k < 0: its
negative, k = 0: the identity), the z of its representation and the multiple of p added to each coordinate's residue."""
import random

import numpy as np

from tests._fp29_ref import MODULUS, R, ints_to_limbs29, limbs29_to_ints

CURVES = (0, 1, 2, 3)                                   # VIMZ_CURVE_BN254_G1, _GRUMPKIN, _PALLAS, _VESTA
CURVE_NAMES = ("bn254_g1", "grumpkin", "pallas", "vesta")
BASE_P = (MODULUS[1], MODULUS[0], MODULUS[2], MODULUS[3])      # coordinate field
ORDER = (MODULUS[0], MODULUS[1], MODULUS[3], MODULUS[2])       # group order (all four curves have prime order)
CURVE_B = (3, -17, 5, 5)
GENERATOR = ((1, 2), (1, 17631683881184975370165255887551781615748388533673675138860), (MODULUS[2] - 1, 2), (MODULUS[3] - 1, 2))
SLOT_WORDS, COORD_WORDS = 40, 10
BOUND_TENTHS = (53, 34, 15, 15)                         # X, Y, ZZ, ZZZ: value·10 < bound·p
MAX_LIFT = (4, 2, 1, 1)                                 # the largest multiple of p a coordinate's residue may carry (ZZ, ZZZ: only on a residue below p/2)
NO_LIFT = (0, 0, 0, 0)
HEAVY_CAP, HEAVY_SPLIT, HEAVY_SPLIT_MIN, HEAVY_PARTS, COMBINE_HEAVY_BLOCKS = 65536, 1024, 2048, 32, 512      # msm_shape.hpp / msm.hpp
HEAVY_GUARD = 64
POOL = 4096


# ---- the four curves, affine, the identity as (0, 0) ------------------------------------------------------------------------------------------
def on_curve(c, pt):
    p = BASE_P[c]
    return pt == (0, 0) or (pt[1] * pt[1] - pt[0] ** 3 - CURVE_B[c]) % p == 0


def neg(c, pt):
    return pt if pt == (0, 0) else (pt[0], (-pt[1]) % BASE_P[c])


def double(c, pt):
    p = BASE_P[c]
    if pt == (0, 0) or pt[1] == 0:
        return (0, 0)
    lam = 3 * pt[0] * pt[0] * pow(2 * pt[1], -1, p) % p
    x = (lam * lam - 2 * pt[0]) % p
    return (x, (lam * (pt[0] - x) - pt[1]) % p)


def add(c, a, b):
    p = BASE_P[c]
    if a == (0, 0):
        return b
    if b == (0, 0):
        return a
    if a[0] == b[0]:
        return double(c, a) if a[1] == b[1] else (0, 0)
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, p) % p
    x = (lam * lam - a[0] - b[0]) % p
    return (x, (lam * (a[0] - x) - a[1]) % p)


_pool = {}


def pool(c, upto=POOL):
    """[k·G for k in 0..upto (at least)] by plain additions; grows on demand (the points that are PACKED come from here)"""
    pts = _pool.setdefault(c, [(0, 0)])
    if len(pts) <= upto:
        g = GENERATOR[c]
        for _ in range(max(upto, POOL) + 1 - len(pts)):
            pts.append(add(c, pts[-1], g))
    return pts


def mul(c, k):
    """k·G for any integer k: the pool for small |k|, double-and-add (Jacobian, one inversion) beyond it — the discrete-log route of the large cases"""
    k %= ORDER[c]
    if k > ORDER[c] // 2:
        return neg(c, mul(c, ORDER[c] - k))
    if k < len(pool(c)):
        return pool(c)[k]
    p, (gx, gy) = BASE_P[c], GENERATOR[c]
    X, Y, Z = gx, gy, 1
    for bit in bin(k)[3:]:
        # doubling (a = 0); a point of odd prime order never has y = 0
        A, B = X * X % p, Y * Y % p
        C = B * B % p
        D = 2 * ((X + B) * (X + B) - A - C) % p
        E = 3 * A % p
        X3 = (E * E - 2 * D) % p
        Y, Z = (E * (D - X3) - 8 * C) % p, 2 * Y * Z % p
        X = X3
        if bit == "1":      # mixed addition of G; the running point is m·G with 2 <= m < order, never ±G
            Z2 = Z * Z % p
            U2, S2 = gx * Z2 % p, gy * Z2 * Z % p
            H, r = (U2 - X) % p, (S2 - Y) % p
            H2 = H * H % p
            H3, V = H * H2 % p, X * H2 % p
            X3 = (r * r - H3 - 2 * V) % p
            Y, Z = (r * (V - X3) - Y * H3) % p, Z * H % p
            X = X3
    zi = pow(Z, -1, p)
    return (X * zi * zi % p, Y * zi * zi * zi % p)


def sum_plain(c, ks):
    """sum of k·G over ks by plain additions of pool points (the small cases' route)"""
    acc = (0, 0)
    for k in ks:
        acc = add(c, acc, pool(c, abs(k))[k] if k >= 0 else neg(c, pool(c, abs(k))[-k]))
    return acc


# ---- slots ------------------------------------------------------------------------------------------------------------------------------------
def slot_values(c, spec):
    """the four integers (X, Y, ZZ, ZZZ) of a spec's slot"""
    k, z, lift = spec
    if k == 0:
        return (0, 0, 0, 0)
    p = BASE_P[c]
    x, y = pool(c, abs(k))[abs(k)]
    if k < 0:
        y = p - y
    zz, zzz = z * z % p, z * z * z % p
    res = (x * zz * R % p, y * zzz * R % p, zz * R % p, zzz * R % p)
    vals = tuple(r + l * p for r, l in zip(res, lift))
    assert res[2] != 0 and all(10 * v < b * p for v, b in zip(vals, BOUND_TENTHS)), "a spec outside the bounds of ec.hpp"
    return vals


def pack(c, specs):
    """specs -> (n, 40) uint32 slots"""
    vals = [v for s in specs for v in slot_values(c, s)]
    out = np.zeros((len(specs), 4, COORD_WORDS), dtype=np.uint32)
    if specs:
        out[:, :, :9] = ints_to_limbs29(vals).reshape(len(specs), 4, 9)
    return out.reshape(len(specs), SLOT_WORDS)


def garbage(n):
    """slots no kernel may read: every word all ones (no limb is below 2^29)"""
    return np.full((n, SLOT_WORDS), 0xffffffff, dtype=np.uint32)


class BadSlot(AssertionError):
    pass


def unpack(c, slot):
    """one slot -> the affine point, after the checks: limbs below 2^29, the bounds of ec.hpp (unless ZZ is literally zero: the identity), ZZ^3 = ZZZ^2, on the curve"""
    w = np.asarray(slot, dtype=np.uint32).reshape(4, COORD_WORDS)
    if (w[:, :9] >> 29).any() or w[:, 9].any():
        raise BadSlot("a limb not below 2^29, or a pad word not zero")
    X, Y, ZZ, ZZZ = limbs29_to_ints(w[:, :9])
    if ZZ == 0:
        return (0, 0)
    p = BASE_P[c]
    for name, v, b in zip("X Y ZZ ZZZ".split(), (X, Y, ZZ, ZZZ), BOUND_TENTHS):
        if 10 * v >= b * p:
            raise BadSlot(f"{name} = {v / p:.3f} p is outside its bound {b / 10} p")
    ri = pow(R, -1, p)
    x, y, zz, zzz = (v * ri % p for v in (X, Y, ZZ, ZZZ))
    if zz == 0 or (zz ** 3 - zzz * zzz) % p:
        raise BadSlot("ZZ^3 != ZZZ^2, or ZZ a non-zero multiple of p")
    inv = pow(zz * zzz, -1, p)
    pt = (x * inv * zzz % p, y * inv * zz % p)
    if not on_curve(c, pt):
        raise BadSlot("not on the curve")
    return pt


def slot_is_identity(slot):
    return not np.asarray(slot).any()


# ---- contents: what every points case is filled with ----------------------------------------------------------------------------------------------
CONTENTS = ("generic", "identity_first_mid_last", "all_identity", "same_point", "same_point_representations", "cancel_pairs", "zero_run_then_more", "max_lifts")


def _small_z(c, rng):
    """a z whose ZZ and ZZZ residues lie below p/2, so that they may carry one p"""
    p = BASE_P[c]
    while True:
        z = rng.randrange(2, p)
        if 2 * (z * z * R % p) < p and 2 * (z * z * z * R % p) < p:
            return z


def _rep(c, rng, k, maximal=False):
    """a random representation of k·G inside the bounds (maximal: every coordinate with its largest lift)"""
    if k == 0:
        return (0, 1, NO_LIFT)
    p = BASE_P[c]
    if maximal:
        return (k, _small_z(c, rng), MAX_LIFT)
    z = rng.choice((1, rng.randrange(2, p)))
    zz, zzz = z * z * R % p, z * z * z * R % p
    return (k, z, (rng.randrange(5), rng.randrange(3), rng.randrange(2) if 2 * zz < p else 0, rng.randrange(2) if 2 * zzz < p else 0))


def content(c, kind, n, seed, kmax=None):
    """n specs of one of CONTENTS; scalars of magnitude at most kmax (default: as small as keeps `generic` distinct, so that small sums stay inside the pool)"""
    rng = random.Random(f"msm-tail/{c}/{kind}/{n}/{seed}")
    if n == 0:
        return []
    kmax = max(kmax or 0, 2 * n if n <= POOL // 2 else n + n // 8, 8)
    distinct = rng.sample(range(1, kmax + 1), n)
    if kind == "generic":
        return [_rep(c, rng, k) for k in distinct]
    if kind == "identity_first_mid_last":
        return [_rep(c, rng, 0 if i in (0, n // 2, n - 1) else k) for i, k in enumerate(distinct)]
    if kind == "all_identity":
        return [_rep(c, rng, 0)] * n
    if kind == "same_point":
        return [_rep(c, rng, distinct[0])] * n
    if kind == "same_point_representations":
        return [_rep(c, rng, distinct[0]) for _ in range(n)]
    if kind == "cancel_pairs":          # slot i holds ±Q by the parity of i's bits: i and i + 2^j (bit j of i clear) are Q and −Q, and so are neighbours 2i, 2i + 1
        return [_rep(c, rng, distinct[0] * (-1 if bin(i).count("1") & 1 else 1)) for i in range(n)]
    if kind == "zero_run_then_more":    # the first half sums to the identity (any prefix of even length does), then more points
        half = (n // 2) & ~1
        return [_rep(c, rng, distinct[i // 2] * (-1 if i & 1 else 1)) if i < half else _rep(c, rng, k) for i, k in enumerate(distinct)]
    if kind == "max_lifts":
        return [_rep(c, rng, k, maximal=True) for k in distinct]
    raise ValueError(kind)


def scalar_sum(specs):
    return sum(s[0] for s in specs)


# ---- quad levels ------------------------------------------------------------------------------------------------------------------------------------
QUAD_COUNTS = (1, 3, 16, 17, 63, 64)
QUAD_TABLES = ("halves", "scattered", "chained")


def quad_table(table, count):
    """(dst, src) of one level: `halves` dst = e, src = e + count; `scattered` a seeded permutation of the 256 slots; `chained` quad e's dst is quad e + 1's src"""
    if table == "halves":
        return list(range(count)), [e + count for e in range(count)]
    perm = random.Random(f"msm-tail/quad/{table}/{count}").sample(range(256), 256)
    if table == "scattered":
        return perm[:count], perm[count:2 * count]
    if table == "chained":
        return perm[:count], perm[1:count + 1]
    raise ValueError(table)


QUAD_LEVEL_CASES = [(count, table) for count in QUAD_COUNTS for table in QUAD_TABLES]
PLANTED = ("copy_left_identity", "right_identity", "both_identity", "generic", "doubling", "doubling_across_representations", "cancellation", "inactive_quad")


def planted_level(c):
    """256 specs and one level whose quads 0..7 — consecutive quads of wave 0 — hold PLANTED in order (count = 7: quad 7 is inactive; its would-be operands
    are slots 7 and 23).  dst = e, src = 16 + e."""
    rng = random.Random(f"msm-tail/planted/{c}")
    specs = content(c, "generic", 256, "planted", kmax=600)
    same = _rep(c, rng, 700)
    put = {0: (0, 11), 1: (12, 0), 2: (0, 0), 3: (13, 14), 4: (same, same), 5: ((15, 1, (4, 2, 0, 0)), _rep(c, rng, 15, maximal=True)), 6: (16, -16)}
    for e, (a, b) in put.items():
        specs[e] = a if isinstance(a, tuple) else _rep(c, rng, a)
        specs[16 + e] = b if isinstance(b, tuple) else _rep(c, rng, b)
    assert specs[5][0] == specs[21][0] and specs[5][1:] != specs[21][1:]
    return specs, (list(range(7)), [16 + e for e in range(7)])


def levels_words(levels):
    """[(dst, src)] -> the hook's (n, 129) uint32: count, dst[64], src[64]"""
    out = np.zeros((len(levels), 129), dtype=np.uint32)
    for i, (dst, src) in enumerate(levels):
        out[i, 0] = len(dst)
        out[i, 1:1 + len(dst)] = dst
        out[i, 65:65 + len(src)] = src
    return out


def apply_levels(specs, slots, levels):
    """what quad_level must leave: per slot (k, limbs) — the scalar of its point and, where the contract fixes the representation (untouched, a source that is
    the identity, a copy into an identity), the exact 40 words; limbs None: a computed sum, any representative inside the bounds"""
    ks = [s[0] for s in specs]
    limbs = [np.array(s) for s in slots]
    for dst, src in levels:
        assert len(set(dst)) == len(dst)
        before_k, before_l = list(ks), list(limbs)
        for d, s in zip(dst, src):
            if before_k[s] == 0:
                continue                            # nothing to store
            if before_k[d] == 0:
                ks[d], limbs[d] = before_k[s], before_l[s]      # copy
            else:
                ks[d] = before_k[d] + before_k[s]
                limbs[d] = None if ks[d] else np.zeros(SLOT_WORDS, dtype=np.uint32)      # a cancellation stores the identity: all zero
    return ks, limbs


TREE256_LEVELS = [(list(range(64)), [e + 128 for e in range(64)]), ([e + 64 for e in range(64)], [e + 192 for e in range(64)])] + \
                 [(list(range(d)), [e + d for e in range(d)]) for d in (64, 32, 16, 8, 4, 2, 1)]

# ---- trees ------------------------------------------------------------------------------------------------------------------------------------------
TREE256_M = (1, 2, 255, 256, 257, 16384)
TREE_ROWS = ((1, 1), (3, 64), (16, 256), (2, 255))      # (count, m)


# ---- scan -------------------------------------------------------------------------------------------------------------------------------------------
SCAN_NB = (1, 1023, 1024, 1025, 7424, 24576)
SCAN_SUB = (8, 16)
SCAN_BLOCKS = (1, 32, 256)
SCAN_HEAVY_MIN = 16
SCAN_COUNTS = ("all_zero", "all_one", "huge_first", "huge_last", "around_multiples_of_sub", "at_heavy_min")
SCAN_CASES = [(nb, kind, sub, blocks) for nb in SCAN_NB for kind in SCAN_COUNTS for sub in SCAN_SUB for blocks in SCAN_BLOCKS]
SCAN_OVERFLOW = {"nb": 1 << 17, "heavy": HEAVY_CAP + 1, "sub": 8, "blocks": 1}


def scan_counts(nb, kind, sub, heavy_min=SCAN_HEAVY_MIN):
    c = np.zeros(nb, dtype=np.uint32)
    if kind == "all_one":
        c[:] = 1
    elif kind == "huge_first":
        c[0] = (1 << 22) + 3
    elif kind == "huge_last":
        c[nb - 1] = (1 << 22) + 3
    elif kind == "around_multiples_of_sub":         # k·sub − 1, k·sub, k·sub + 1 for k = 1, 2, 3, ... bucket after bucket
        i = np.arange(nb)
        c[:] = (1 + (i // 3) % 5) * sub + (i % 3) - 1
    elif kind == "at_heavy_min":                    # exactly heavy_min sub-buckets (not heavy) and heavy_min + 1 (heavy), among light ones
        i = np.arange(nb)
        c[:] = np.where(i % 7 == 0, heavy_min * sub, np.where(i % 7 == 3, heavy_min * sub + 1, i % 5))
    elif kind != "all_zero":
        raise ValueError(kind)
    return c


def scan_overflow_counts():
    o = SCAN_OVERFLOW
    c = np.full(o["nb"], 2, dtype=np.uint32)
    c[:o["heavy"]] = SCAN_HEAVY_MIN * o["sub"] + 1
    return c


def split_over_blocks(counts, blocks):
    """(blocks, nb) histograms that sum to counts, unevenly: block k takes count // blocks, the first count % blocks blocks (from a bucket-dependent start) one more"""
    nb = len(counts)
    k = np.arange(blocks, dtype=np.uint32)[:, None]
    start = (np.arange(nb, dtype=np.uint32) * 7)[None, :]
    hist = counts[None, :] // blocks + (((k + start) % blocks) < (counts[None, :] % blocks))
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    assert np.array_equal(hist.sum(axis=0, dtype=np.uint64), counts)
    return hist


def scan_ref(hist, sub, heavy_min):
    """counts, bucket_off, sub_off (exclusive, nb + 1), the heavy set, the per-block exclusive prefixes"""
    hist = np.asarray(hist, dtype=np.uint64)
    counts = hist.sum(axis=0)
    m = (counts + sub - 1) // sub
    boff = np.concatenate([[0], np.cumsum(counts)])
    soff = np.concatenate([[0], np.cumsum(m)])
    prefixes = np.cumsum(hist, axis=0) - hist
    return counts, boff, soff, set(np.nonzero(m > heavy_min)[0].tolist()), prefixes


# ---- combine ----------------------------------------------------------------------------------------------------------------------------------------
COMBINE_LANE_BITS = (0, 1, 2, 3, 4)
COMBINE_ALL_CURVES_LANE_BITS = 1


def heavy_min_of(lane_bits):
    return 16 << lane_bits                            # as msm_shape sets it: 16 partials a lane


def ordinary_sizes(lane_bits):
    L = 1 << lane_bits
    return sorted({0, 1, 2, L - 1, L, L + 1, 2 * L + 1, heavy_min_of(lane_bits)})


def combine_ordinary_layout(lane_bits, row=0):
    """bucket sizes m[b] (all <= heavy_min): workgroup 0 runs through ordinary_sizes, its LAST bucket a large one; workgroup 1 has nothing to fold (sizes 0 and 1
    only: the early return); workgroup 2 runs through the sizes from another start; then a part of a workgroup (nb is no multiple of the buckets per workgroup)
    that ends on a bucket of heavy_min partials.  `row` rotates the sizes."""
    per_wg, sizes = 256 >> lane_bits, ordinary_sizes(lane_bits)
    L = 1 << lane_bits
    m = [sizes[(b + row) % len(sizes)] for b in range(per_wg)]
    m[per_wg - 1] = 2 * L + 1
    m += [(b + row) & 1 for b in range(per_wg)]
    m += [sizes[(3 * b + 1 + row) % len(sizes)] for b in range(per_wg)]
    m += [sizes[(b + 2 + row) % len(sizes)] for b in range(5)] + [heavy_min_of(lane_bits)]
    return m


# name -> (lane_bits, rows, calls, kind); kind selects the layout (combine_sizes).  The ordinary buckets and the heavy sizes run at every lane_bits (the ordinary
# lanes and heavy_min depend on it); the list of 513, the split buckets and the overflowed list — workgroups that do not look at lane_bits — at 0 and 1 or at 1, the
# value at which all four curves run.
COMBINE_CASES = {}
for _lb in COMBINE_LANE_BITS:
    COMBINE_CASES[f"ordinary/lane_bits={_lb}/rows=1"] = (_lb, 1, 1, "ordinary")
    COMBINE_CASES[f"ordinary/lane_bits={_lb}/rows=3"] = (_lb, 3, 1, "ordinary")
    COMBINE_CASES[f"heavy_sizes/lane_bits={_lb}"] = (_lb, 1, 1, "heavy_sizes")
for _lb in (0, 1):
    COMBINE_CASES[f"heavy_513/lane_bits={_lb}"] = (_lb, 1, 1, "heavy_513")
COMBINE_CASES.update({
    "split_sizes/calls=2": (1, 1, 2, "split_sizes"),
    "split_past_1024/calls=2": (1, 1, 2, "split_past_1024"),
    "split_at_0/calls=2": (1, 1, 2, "split_at_0"),
    "split_rows=3/calls=2": (1, 3, 2, "split_sizes"),
    "overflowed_list": (1, 1, 1, "overflow"),
})
HEAVY_SIZES = lambda lane_bits: (heavy_min_of(lane_bits) + 1, 255, 256, 257, 2047)      # noqa: E731
SPLIT_SIZES = (2048, 2049, 4097)
OVERFLOW_SIZES = (17, 300, 2048)


def combine_sizes(name, row=0):
    """(bucket sizes m[b], heavy ids in list order, heavy count word) of a case's row"""
    lane_bits, _, _, kind = COMBINE_CASES[name]
    hm = heavy_min_of(lane_bits)
    few = [(b + row) % 3 for b in range(7)]                  # light buckets around the heavy ones
    if kind == "ordinary":
        return combine_ordinary_layout(lane_bits, row), [], 0
    if kind == "heavy_sizes":
        m = []
        for s in HEAVY_SIZES(lane_bits):
            m += few + [s]
        m += few
        ids = [b for b, s in enumerate(m) if s > hm]
        return m, ids[::-1], len(ids)                        # (the list's order comes from an atomic: any order)
    if kind == "heavy_513":
        m = [hm + 1 if b % 2 else b % 3 for b in range(2 * (COMBINE_HEAVY_BLOCKS + 1))]
        ids = [b for b, s in enumerate(m) if s > hm]
        assert len(ids) == COMBINE_HEAVY_BLOCKS + 1
        return m, ids, len(ids)
    if kind == "split_sizes":
        sizes = SPLIT_SIZES[row % 3:] + SPLIT_SIZES[:row % 3]
        m = []
        for s in sizes:
            m += few + [s]
        m += few + [hm + 1]
        ids = [b for b, s in enumerate(m) if s > hm]
        return m, ids, len(ids)
    if kind in ("split_past_1024", "split_at_0"):            # 1025 heavy buckets, one of them of 2048 partials: past MSM_HEAVY_SPLIT one workgroup folds it, at 0 two stages
        m = [hm + 1] * HEAVY_SPLIT + [2, HEAVY_SPLIT_MIN, 1]
        big = HEAVY_SPLIT + 1
        ids = list(range(HEAVY_SPLIT))
        ids = ids + [big] if kind == "split_past_1024" else [big] + ids
        return m, ids, len(ids)
    if kind == "overflow":                                   # the count word says the list overflowed: every bucket is folded by its ordinary lanes
        m = []
        for s in OVERFLOW_SIZES:
            m += few + [s]
        return m, [], HEAVY_CAP + 1
    raise ValueError(kind)


def bucket_specs(c, m, seed):
    """the partials of buckets of sizes m: the contents rotate over the buckets, shifted after every eight so that a size that recurs meets another content; a
    bucket of more than 64 partials takes the next of BIG_CONTENTS — never all identities, whose first partial already is the sum"""
    out, big, h = [], 0, hash_int(seed)
    for b, s in enumerate(m):
        if s > 64:
            kind, big = BIG_CONTENTS[(big + h) % len(BIG_CONTENTS)], big + 1
        else:
            kind = CONTENTS[(b + b // 8 + h) % len(CONTENTS)]
        out.append(content(c, kind, s, f"{seed}/{b}"))
    return out


BIG_CONTENTS = tuple(k for k in CONTENTS if k != "all_identity")


def combine_specs(c, name, row):
    """the partials of a combine case's row, bucket by bucket (the two cases over 1025 heavy buckets share theirs: only the list's order differs)"""
    seed = "split_1025" if COMBINE_CASES[name][3] in ("split_past_1024", "split_at_0") else name
    return seed, lambda: bucket_specs(c, combine_sizes(name, row)[0], f"{seed}/{row}")


def hash_int(s):
    return sum(str(s).encode()) % 97


# ---- reduce -----------------------------------------------------------------------------------------------------------------------------------------
REDUCE_NBW = (2, 16, 128, 256, 512, 1024, 2048)
REDUCE_ALL_CURVES_NBW = 1024
REDUCE_BUCKETS = ("all_empty", "only_bucket_0", "only_top_bucket", "only_first_of_last_chunk", "every_bucket_same_point", "alternating_q_minus_q", "full_distinct",
                  "zero_counts_over_garbage")
REDUCE_SHAPES = ((1, 1), (3, 1), (1, 3), (3, 3))        # (windows, rows)
REDUCE_MODE1_WINDOWS = (1, 2, 16)
REDUCE_PLANES_NBW = (1024, 4096, 16384, 32768)
REDUCE_PLANES_G = (1, 4, 16, 8)


def reduce_cases(nbw):
    """[(windows, rows, kinds)]: kinds[r][w] the bucket content of window w of row r — every kind alone (one window, one row), then the larger shapes over rotating kinds"""
    cases = [(1, 1, [[k]]) for k in REDUCE_BUCKETS]
    for i, (W, Rr) in enumerate(REDUCE_SHAPES[1:]):
        cases.append((W, Rr, [[REDUCE_BUCKETS[(3 * i + 3 * r + w) % len(REDUCE_BUCKETS)] for w in range(W)] for r in range(Rr)]))
    return cases


def window_specs(c, kind, nbw, seed):
    """(specs of the nbw buckets' sums, counts): a bucket with count 0 is EMPTY whatever its spec says (zero_counts_over_garbage: its slot is garbage)"""
    rng = random.Random(f"msm-tail/reduce/{c}/{kind}/{nbw}/{seed}")
    T = min(256, nbw)
    ch = nbw // T
    ident = (0, 1, NO_LIFT)
    specs, counts = [ident] * nbw, [0] * nbw
    only = {"only_bucket_0": 0, "only_top_bucket": nbw - 1, "only_first_of_last_chunk": (T - 1) * ch}
    if kind in only:
        specs[only[kind]], counts[only[kind]] = _rep(c, rng, rng.randrange(1, POOL)), 1 + rng.randrange(40)
    elif kind == "every_bucket_same_point":
        specs, counts = [_rep(c, rng, 77)] * nbw, [3] * nbw
    elif kind == "alternating_q_minus_q":
        specs, counts = [_rep(c, rng, 91 if i % 2 == 0 else -91) for i in range(nbw)], [1] * nbw
    elif kind == "full_distinct":
        specs, counts = content(c, "generic", nbw, seed), [1 + i % 50 for i in range(nbw)]
    elif kind == "zero_counts_over_garbage":        # every third bucket is empty over a garbage slot; a filled bucket may hold the identity
        gen = content(c, "identity_first_mid_last", nbw, seed)
        specs, counts = [g if i % 3 else ident for i, g in enumerate(gen)], [1 if i % 3 else 0 for i in range(nbw)]
    elif kind != "all_empty":
        raise ValueError(kind)
    return specs, counts


def reduce_ref(ks, counts):
    """(weighted, plain) scalars of one window: sum (idx + 1)·k_idx and sum k_idx over the filled buckets"""
    live = [k if n else 0 for k, n in zip(ks, counts)]
    run = weighted = 0
    for k in reversed(live):                         # running sums, as the kernel's chunks do: sum_j (j + 1) k_j = sum of the suffix sums
        run += k
        weighted += run
    return weighted, sum(live)


def planes_ref(ks, counts):
    """the P + 2 scalars k_reduce_planes writes: plane p = sum over the buckets whose index has bit p set, then the plain sums of the low and the high half"""
    nbw = len(ks)
    P = nbw.bit_length() - 1
    live = [k if n else 0 for k, n in zip(ks, counts)]
    return [sum(k for g, k in enumerate(live) if (g >> p) & 1) for p in range(P)] + [sum(live[:nbw // 2]), sum(live[nbw // 2:])]


def planes_total(scalars):
    """sum (g + 1) k_g from the P + 2 plane scalars, as msm_finish weighs them"""
    P = len(scalars) - 2
    return sum(s << p for p, s in enumerate(scalars[:P])) + scalars[P] + scalars[P + 1]


def bucket_layout(counts, garbage_every=3):
    """sub_off of a reduce case: bucket g owns 1 + g % 3 slots whatever its count (only the first is ever read); returns (sub_off, first slots)"""
    width = [1 + g % garbage_every for g in range(len(counts))]
    soff = np.concatenate([[0], np.cumsum(width)]).astype(np.uint32)
    return soff, soff[:-1]


# ---- invalid layouts: one refusal per validation rule of the hooks -----------------------------------------------------------------------------------
INVALID = ("offsets_not_monotone", "offsets_outside_the_array", "bucket_id_not_below_nb", "index_not_below_256", "dst_twice_in_a_level", "nbw_not_a_power_of_two",
           "nbw_above_32768", "rows_above_16")


# ---- the groups of the GPU test: group -> its cases, in the order the driver runs them (tests/_msm_tail_gpu.py runs every case of a group and prints how many
# it ran; tests/test_gpu_msm_tail.py holds that count against these lists) ---------------------------------------------------------------------------------
def group_cases(group):
    if group == "quad_level":       # every case over all CONTENTS at once (one workgroup each); the planted level on its own slots
        return [(c, count, table) for c in CURVES for count, table in QUAD_LEVEL_CASES] + [(c, "planted", "planted") for c in CURVES]
    if group == "quad_tree":
        return [(c, kind) for c in CURVES for kind in CONTENTS]
    if group == "tree256":
        return [(c, m, kind) for c in CURVES for m in TREE256_M for kind in CONTENTS]
    if group == "tree_rows":
        return [(c, count, m) for c in CURVES for count, m in TREE_ROWS]
    if group == "scan":             # every case through k_prefix_scan and through k_scan
        return list(SCAN_CASES) + [("overflow",)]
    if group == "combine":
        return [(c, name) for c in CURVES for name, (lb, _, _, _) in COMBINE_CASES.items() if c == 0 or lb == COMBINE_ALL_CURVES_LANE_BITS]
    if group == "reduce":
        return [(c, nbw, W, Rr, tuple(tuple(r) for r in kinds)) for c in CURVES for nbw in REDUCE_NBW if c == 0 or nbw == REDUCE_ALL_CURVES_NBW
                for W, Rr, kinds in reduce_cases(nbw)]
    if group == "reduce_plain":     # mode 1 at nbw = 1024: the virtual windows of a shared bucket set, weighted and plain sums
        return [(c, V) for c in CURVES for V in REDUCE_MODE1_WINDOWS]
    if group == "reduce_planes":    # mode 2, calls = 2
        return [(c, nbw) for c in CURVES for nbw in REDUCE_PLANES_NBW if c == 0 or nbw == REDUCE_ALL_CURVES_NBW]
    if group == "invalid":
        return list(INVALID)
    raise ValueError(group)


GROUPS = ("quad_level", "quad_tree", "tree256", "tree_rows", "scan", "combine", "reduce", "reduce_plain", "reduce_planes", "invalid")
