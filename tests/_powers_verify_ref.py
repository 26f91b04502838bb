"""Judging a powers-of-tau string (vimz_powers_verify; vimz_amd/csrc/g16_powers_verify.hip) stated in plain Python on tests/_pairing.py's arithmetic, and the cases
the CPU loop of the kernels' functions (tests/test_powers_verify_host.py) and the GPU tests (tests/test_gpu_powers_verify.py) run.  A G1 point is (x, y), a G2
point ((x.c0, x.c1), (y.c0, y.c1)), the identity all zeros — the library's encoding.  No GPU, no numpy.  Checked by tests/test_powers_verify_ref_host.py.  Test
infrastructure."""
import functools
import random

from tests import _pairing as bp
from tests._pairing import Q, R

RLC_CHUNK = 8                    # pairs of one thread of k_powers_rlc (g16_point_stage.hpp)
PT_BLOCK = 64                    # threads of a block
COORD, OFF_CURVE, IDENTITY, SUBGROUP, FIRST, RATIO_TAU_G1, RATIO_ALPHA_G1, RATIO_BETA_G1, RATIO_TAU_G2, HALVES, BETA = (1 << k for k in range(11))      # VIMZ_POWERS_*
ARRAYS = (None, "tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")      # first_bad's array numbers
GROUP = {"tau_g1": 1, "tau_g2": 2, "alpha_g1": 1, "beta_g1": 1, "beta_g2": 2}
G1_ZERO, G2_ZERO = (0, 0), ((0, 0), (0, 0))
COFACTOR = 2 * Q - R             # of the twist: #E'(Fq2) = r·(2q − r)
SMALL_FACTORS = (10069, 5864401)


# ---- Fq2 and the twist beyond what _pairing.py has ----------------------------------------------------------------------------------------------
def f2_pow(a, e):
    acc = (1, 0)
    while e:
        if e & 1:
            acc = bp._f2_mul(acc, a)
        a = bp._f2_mul(a, a)
        e >>= 1
    return acc


def f2_sqrt(a):
    """a square root of a in Fq2 = Fq[u]/(u² + 1), q ≡ 3 mod 4 (Adj, Rodríguez-Henríquez, algorithm 9), or None"""
    if a == (0, 0):
        return a
    a1 = f2_pow(a, (Q - 3) // 4)
    alpha = bp._f2_mul(bp._f2_mul(a1, a1), a)
    a0 = bp._f2_mul((alpha[0], -alpha[1] % Q), alpha)      # alpha^q · alpha: the norm
    if a0 == (Q - 1, 0):
        return None
    x0 = bp._f2_mul(a1, a)
    if alpha == (Q - 1, 0):
        return bp._f2_mul((0, 1), x0)
    b = f2_pow(((1 + alpha[0]) % Q, alpha[1]), (Q - 1) // 2)
    return bp._f2_mul(b, x0)


def twist_point(x):
    """the point of the twist y² = x³ + 3/(9 + u) with that x, or None"""
    x3 = bp._f2_mul(bp._f2_mul(x, x), x)
    y = f2_sqrt(((x3[0] + bp.B2[0]) % Q, (x3[1] + bp.B2[1]) % Q))
    return None if y is None else (x, y)


def g2_mul_raw(p, k):
    """k·p by double-and-add WITHOUT reducing k (bp.g2_mul reduces mod r, which is only right inside the subgroup)"""
    r = None
    while k:
        if k & 1:
            r = bp.g2_add(r, p)
        p = bp.g2_add(p, p)
        k >>= 1
    return r


@functools.lru_cache(maxsize=None)
def outside_points():
    """points of the twist outside the subgroup of order r: `a` = the point with x = (1, 0); `small` = T = [(2q − r)·r / 10069]·a, of order 10069; `mixed` =
    [5]G2 + T, which a check on a SUM of points would miss once in 10069 tries"""
    a = twist_point((1, 0))
    t = g2_mul_raw(a, COFACTOR * R // SMALL_FACTORS[0])
    return {"a": a, "small": t, "mixed": bp.g2_add(bp.g2_mul(bp.G2, 5), t)}


# ---- encodings ------------------------------------------------------------------------------------------------------------------------------------
def enc(group, p):
    return (G1_ZERO if group == 1 else G2_ZERO) if p is None else p


def dec(group, p):
    return None if p == (G1_ZERO if group == 1 else G2_ZERO) else p


def mul(group, k):
    return enc(group, bp.g1_mul(bp.G1, k) if group == 1 else bp.g2_mul(bp.G2, k))


def flat(group, p):
    return list(p) if group == 1 else [p[0][0], p[0][1], p[1][0], p[1][1]]


# ---- the verdict ----------------------------------------------------------------------------------------------------------------------------------
def point_flags(group, p):
    """what k_powers_flags (and the host's range check) says of one point"""
    if max(flat(group, p)) >= Q:
        return COORD
    if dec(group, p) is None:
        return IDENTITY
    if not (bp.g1_on_curve(p) if group == 1 else bp.g2_on_curve(p)):
        return OFF_CURVE
    if group == 2 and g2_mul_raw(p, R) is not None:
        return SUBGROUP
    return 0


def rlc_points(group, points, rho):
    """S = Σ rho_i·P_i, S' = Σ rho_i·P_(i+1) over i < len(points) − 1, on points of the group (every one in the subgroup)"""
    add, pmul = (bp.g1_add, bp.g1_mul) if group == 1 else (bp.g2_add, bp.g2_mul)
    s = s1 = None
    for i in range(len(points) - 1):
        s, s1 = add(s, pmul(dec(group, points[i]), rho[i])), add(s1, pmul(dec(group, points[i + 1]), rho[i]))
    return s, s1


def judge(string, rho):
    """(result, first_bad) of a string {"tau_g1": [..], "tau_g2", "alpha_g1", "beta_g1", "beta_g2": [point]} with the pairs' scalars rho (len(tau_g1) − 1 of them)"""
    for number in range(1, 6):
        name = ARRAYS[number]
        f = [point_flags(GROUP[name], p) for p in string[name]]
        if any(f):
            bits = 0
            for x in f:
                bits |= x
            return bits, (number, next(i for i, x in enumerate(f) if x))
    if string["tau_g1"][0] != bp.G1:
        return FIRST, (1, 0)
    if string["tau_g2"][0] != bp.G2:
        return FIRST, (2, 0)
    result = 0
    tau2_1 = string["tau_g2"][1]
    for name, bit in (("tau_g1", RATIO_TAU_G1), ("alpha_g1", RATIO_ALPHA_G1), ("beta_g1", RATIO_BETA_G1)):
        s, s1 = rlc_points(1, string[name], rho)
        if not bp.pairing_product_is_one([(s1, bp.G2), (bp.g1_neg(s), tau2_1)]):
            result |= bit
    d, d1 = rlc_points(2, string["tau_g2"], rho)
    if not bp.pairing_product_is_one([(bp.G1, d1), (bp.g1_neg(string["tau_g1"][1]), d)]):
        result |= RATIO_TAU_G2
    if not bp.pairing_product_is_one([(string["tau_g1"][1], bp.G2), (bp.g1_neg(bp.G1), tau2_1)]):
        result |= HALVES
    if not bp.pairing_product_is_one([(string["beta_g1"][0], bp.G2), (bp.g1_neg(bp.G1), string["beta_g2"][0])]):
        result |= BETA
    return result, (0, 0)


def string_points(scalars):
    """a string of points from tests/_g16_powers_ref.string_scalars' scalars"""
    return {name: [mul(GROUP[name], s) for s in scalars[name]] for name in ARRAYS[1:]}


# ---- the combination on SCALARS (a point [s]G is its s), as the kernel cuts it -------------------------------------------------------------------
def rlc_scalars(s, rho):
    n_pairs = len(rho)
    assert len(s) >= n_pairs + 1
    return sum(rho[i] * s[i] for i in range(n_pairs)) % R, sum(rho[i] * s[i + 1] for i in range(n_pairs)) % R


def rlc_chunk_scalars(s, rho, shift):
    """the chunk sums k_powers_rlc leaves for the reduction: thread t owns the pairs RLC_CHUNK·t .. of the pass with that shift"""
    n_pairs = len(rho)
    return [sum(rho[i] * s[i + shift] for i in range(lo, min(lo + RLC_CHUNK, n_pairs))) % R for lo in range(0, n_pairs, RLC_CHUNK)]


# ---- the cases of the combination ----------------------------------------------------------------------------------------------------------------
BASE_N = PT_BLOCK * RLC_CHUNK + 2                          # points: pairs up to one block of chunks and one more
BASE_D = 0x1F3D5B79A1C3E5F7092B4D6F81A3C5E7 % R
RLC_PAIRS = {1: (1, RLC_CHUNK - 1, RLC_CHUNK, RLC_CHUNK + 1, PT_BLOCK * RLC_CHUNK - 1, PT_BLOCK * RLC_CHUNK, PT_BLOCK * RLC_CHUNK + 1),
             2: (1, RLC_CHUNK, RLC_CHUNK + 1, PT_BLOCK * RLC_CHUNK + 1)}
MAX128 = (1 << 128) - 1


def base_scalars():
    """s_k = d·(C + k), C = RLC_CHUNK, but s_C = −2·s_0: with rho_0 = 2k, rho_C = k the first two chunks' sums are OPPOSITE points; s_(C+1) = (2C + 1)·d and
    s_(2C) = 3C·d give chunks 1 and 2 EQUAL sums with rho_(C+1) = 3C·k, rho_(2C) = (2C + 1)·k"""
    s = [BASE_D * (RLC_CHUNK + k) % R for k in range(BASE_N)]
    s[RLC_CHUNK] = (R - 2 * s[0]) % R
    return s


def base_line(group):
    """the native program's BASE line"""
    return f"BASE {group} {BASE_N} {BASE_D * RLC_CHUNK % R:x} {BASE_D:x} {RLC_CHUNK}:{base_scalars()[RLC_CHUNK]:x}"


def rlc_cases(group):
    """name -> rho (its length is the number of pairs; the points are the first len + 1 of base_scalars): every size with random scalars; the patterns — all zero
    (S and S' are the identity), all one, all 2^128 − 1, a single non-zero rho at the last pair — at the sizes of one pair, a chunk and one more, and the largest;
    two chunk sums opposite (and a third chunk after them), two equal: the reduction's cancellation and doubling"""
    C = RLC_CHUNK
    cases = {}
    for n_pairs in RLC_PAIRS[group]:
        rng = random.Random(f"rlc/{group}/{n_pairs}")
        rho = [rng.getrandbits(128) for _ in range(n_pairs)]
        if n_pairs > 2:
            rho[1] = 0                                     # a zero among the random ones
        cases[f"{n_pairs}/random"] = rho
        if n_pairs in (1, C + 1, PT_BLOCK * C + 1):
            cases[f"{n_pairs}/zero"] = [0] * n_pairs
            cases[f"{n_pairs}/one"] = [1] * n_pairs
            cases[f"{n_pairs}/max"] = [MAX128] * n_pairs
            cases[f"{n_pairs}/last"] = [0] * (n_pairs - 1) + [rng.getrandbits(128) | 1]
        if n_pairs >= C + 1:
            k = rng.getrandbits(100) | 1
            opp = [0] * n_pairs
            opp[0], opp[C] = 2 * k, k
            if n_pairs > 2 * C:
                opp[n_pairs - 1] = rng.getrandbits(128) | 1      # the sum restarts after the cancellation
            cases[f"{n_pairs}/opposite"] = opp
        if n_pairs >= 2 * C + 1:
            k = rng.getrandbits(100) | 1
            eq = [0] * n_pairs
            eq[C + 1], eq[2 * C] = 3 * C * k, (2 * C + 1) * k
            cases[f"{n_pairs}/equal"] = eq
    return cases


# ---- the cases of the per-point flags ------------------------------------------------------------------------------------------------------------
FLAGS_N = (63, 64, 65)


def bad_points(group):
    """kind -> (point, its flag): y + 1, x = q, the identity, and in G2 the three points outside the subgroup"""
    if group == 1:
        g = mul(1, 12345)
        return {"y_plus_1": ((g[0], (g[1] + 1) % Q), OFF_CURVE), "x_is_q": ((Q, g[1]), COORD), "identity": (G1_ZERO, IDENTITY)}
    g = mul(2, 12345)
    out = {"y_plus_1": ((g[0], ((g[1][0] + 1) % Q, g[1][1])), OFF_CURVE), "x_is_q": (((g[0][0], Q), g[1]), COORD), "identity": (G2_ZERO, IDENTITY)}
    out.update({name: (p, SUBGROUP) for name, p in outside_points().items()})
    return out


def flags_cases(group):
    """name -> (scalars of the good points, {index: kind}): n in FLAGS_N, one bad point at index 0, at n/2 and at n − 1, the kinds rotated over the three places
    so that every kind stands at every place once"""
    kinds = sorted(bad_points(group))
    cases = {}
    for n in FLAGS_N:
        s = [(BASE_D * (7 + k)) % R for k in range(n)]
        for rot in range(len(kinds)):
            cases[f"{n}/{rot}"] = (s, {pos: kinds[(rot + j) % len(kinds)] for j, pos in enumerate((0, n // 2, n - 1))})
    return cases
