"""The device Miller loop (vimz_amd/csrc/pairing_stage.hpp: miller_thread, what one thread of k_miller does) and the batch equation of vimz_decider_verify_batch
(vimz_amd/csrc/decider_batch.hpp) restated in plain Python integers.  Test infrastructure only: nothing of the product imports this.

The tower is pairing.hpp's: Fq2 = Fq[u]/(u² + 1), Fq6 = Fq2[v]/(v³ − ξ), ξ = 9 + u, Fq12 = Fq6[w]/(w² − v) — held here as six Fq2 coefficients of 1, w, .., w⁵ with
w⁶ = ξ.  T runs in homogeneous projective coordinates (X : Y : Z) of the twist y² = x³ + b', b' = 3/ξ, with no inversion; each step multiplies f by a line with
three non-zero Fq2 coefficients, at 1, w and w³:

    doubling   B = Y², C = Z², E = 3b'·C, F = 3E, H = 2YZ, J = X²:     line (H·yP, −3J·xP, B − E);   T <- (2XY·(B − F), (B + F)² − 12E², 4B·H)
    addition   θ = Y − yQ·Z, λ = X − xQ·Z:                            line (λ·yP, −θ·xP, θ·xQ − λ·yQ)
               C = θ², D = λ², E = λD, F = ZC, G = XD, H = E + F − 2G:  T <- (λH, θ(G − H) − E·Y, Z·E)

over the 64 bits of 6t + 2 below its leading one, then the additions of π(Q) and −π²(Q).  These lines are the affine lines of pairing.hpp::miller_loop times 2YZ
and times λ — factors in Fq2 the final exponentiation removes — so the VALUE differs from the host's word for word while the pairing is the same.
`words` is the kernel's output: the 12 Fq coefficients in the order of the struct (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 = the coefficients of 1, w², w⁴, w, w³, w⁵;
real part first), canonical, 8 little-endian 32-bit words each."""
from tests import _pairing as bp

Q, R = bp.Q, bp.R
ATE_LOW = bp.ATE_LOOP_COUNT - (1 << 64)      # the 64 bits below the leading one
XI = (9, 1)


def f2_add(a, b):
    return (a[0] + b[0]) % Q, (a[1] + b[1]) % Q


def f2_sub(a, b):
    return (a[0] - b[0]) % Q, (a[1] - b[1]) % Q


def f2_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q


def f2_scale(a, k):
    return a[0] * k % Q, a[1] * k % Q


def f2_neg(a):
    return -a[0] % Q, -a[1] % Q


def f2_conj(a):
    return a[0], -a[1] % Q


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


B_TWIST = bp.B2                                  # 3/ξ
G12 = f2_pow(XI, (Q - 1) // 3)
G13 = f2_pow(XI, (Q - 1) // 2)
F12_ONE = ((1, 0),) + ((0, 0),) * 5


def f12_mul(a, b):
    """six Fq2 coefficients of 1, w, .., w⁵; w⁶ = ξ"""
    t = [(0, 0)] * 11
    for i, x in enumerate(a):
        if x != (0, 0):
            for j, y in enumerate(b):
                t[i + j] = f2_add(t[i + j], f2_mul(x, y))
    return tuple(f2_add(t[k], f2_mul(XI, t[k + 6])) if k < 5 else t[k] for k in range(6))


def line(l0, l1, l3):
    return (l0, l1, (0, 0), l3, (0, 0), (0, 0))


def step_double(f, T, P):
    X, Y, Z = T
    B, C, J = f2_mul(Y, Y), f2_mul(Z, Z), f2_mul(X, X)
    E = f2_scale(f2_mul(B_TWIST, C), 3)
    F = f2_scale(E, 3)
    H = f2_scale(f2_mul(Y, Z), 2)
    f = f12_mul(f, line(f2_scale(H, P[1]), f2_neg(f2_scale(J, 3 * P[0])), f2_sub(B, E)))
    BF = f2_add(B, F)
    T = (f2_mul(f2_scale(f2_mul(X, Y), 2), f2_sub(B, F)), f2_sub(f2_mul(BF, BF), f2_scale(f2_mul(E, E), 12)), f2_scale(f2_mul(B, H), 4))
    return f, T


def step_add(f, T, Qa, P):
    X, Y, Z = T
    theta, lam = f2_sub(Y, f2_mul(Qa[1], Z)), f2_sub(X, f2_mul(Qa[0], Z))
    f = f12_mul(f, line(f2_scale(lam, P[1]), f2_neg(f2_scale(theta, P[0])), f2_sub(f2_mul(theta, Qa[0]), f2_mul(lam, Qa[1]))))
    C, D = f2_mul(theta, theta), f2_mul(lam, lam)
    E = f2_mul(lam, D)
    F, G = f2_mul(Z, C), f2_mul(X, D)
    H = f2_sub(f2_add(E, F), f2_scale(G, 2))
    return f, (f2_mul(lam, H), f2_sub(f2_mul(theta, f2_sub(G, H)), f2_mul(E, Y)), f2_mul(Z, E))


def miller(q2, p1):
    """q2: ((x.c0, x.c1), (y.c0, y.c1)) or None, p1: (x, y) or None -> six Fq2 coefficients"""
    if q2 is None or p1 is None:
        return F12_ONE
    f, T = F12_ONE, (q2[0], q2[1], (1, 0))
    for i in range(63, -1, -1):
        f = f12_mul(f, f)
        f, T = step_double(f, T, p1)
        if (ATE_LOW >> i) & 1:
            f, T = step_add(f, T, q2, p1)
    q1 = (f2_mul(f2_conj(q2[0]), G12), f2_mul(f2_conj(q2[1]), G13))
    nq2 = (f2_mul(f2_conj(q1[0]), G12), f2_neg(f2_mul(f2_conj(q1[1]), G13)))
    f, T = step_add(f, T, q1, p1)
    f, T = step_add(f, T, nq2, p1)
    return f


STRUCT_ORDER = (0, 2, 4, 1, 3, 5)      # the power of w each Fq2 of the struct (c0.c0 .. c1.c2) multiplies


def words(f):
    out = []
    for k in STRUCT_ORDER:
        for c in f[k]:
            out.extend((c >> (32 * i)) & 0xFFFFFFFF for i in range(8))
    return out


def from_words(w):
    el = [sum(int(w[8 * j + i]) << (32 * i) for i in range(8)) for j in range(12)]
    f = [None] * 6
    for s, k in enumerate(STRUCT_ORDER):
        f[k] = (el[2 * s], el[2 * s + 1])
    return tuple(f)


def to_pairing_basis(f):
    """a + b·u at w^k is (a − 9b)·w^k + b·w^(k+6) in tests/_pairing.py's Fq[w]/(w¹² − 18w⁶ + 82)"""
    return bp.f12([(f[k][0] - 9 * f[k][1]) for k in range(6)] + [f[k][1] for k in range(6)])


# ---- the batch equation of vimz_decider_verify_batch over tests/_pairing.py and tests/_novadecider.py -------------------------------------------------------------
def batch_pairs(key, items, scalars):
    """items: [(steps, z0, z_i, words)] that pass the per-proof stage, scalars: [(rho, sigma, sigma')] -> the pairs [(G1 point or None, G2 point)] whose product
    of pairings is one iff the chunk is accepted: the n pairs (−rho_i·A_i, B_i), then alpha/beta, vk_x/gamma, C/delta, the KZG pair of VK and that of G_2."""
    from tests import _novadecider as nd
    g, kz = key["groth16"], key["kzg"]
    n_pub = len(g["ic"]) - 1
    pairs, rho_sum, pub_sum, y_sum = [], 0, [0] * n_pub, 0
    c_sum = vk_sum = g2_sum = None
    for (steps, z0, zi, w), (rho, sig, sig2) in zip(items, scalars):
        p = [int(x) for x in w]
        pub, cmW, cmE = nd.public_inputs(key, steps, z0, zi, p)
        A, C, piW, piE = (p[9], p[10]), (p[15], p[16]), (p[21], p[22]), (p[23], p[24])
        B = ((p[12], p[11]), (p[14], p[13]))
        pairs.append((bp.g1_mul(bp.g1_neg(A), rho), B))
        rho_sum = (rho_sum + rho) % R
        pub_sum = [(s + rho * x) % R for s, x in zip(pub_sum, pub)]
        c_sum = bp.g1_add(c_sum, bp.g1_mul(C, rho))
        vk_sum = bp.g1_add(vk_sum, bp.g1_add(bp.g1_mul(piW, sig), bp.g1_mul(piE, sig2)))
        for s, x, pi, cm in ((sig, p[17], piW, cmW), (sig2, p[18], piE, cmE)):
            g2_sum = bp.g1_add(g2_sum, bp.g1_mul(bp.g1_neg(pi), s * x % R))
            g2_sum = bp.g1_add(g2_sum, bp.g1_mul(bp.g1_neg(nd._g1(cm)), s))
        y_sum = (y_sum + sig * p[19] + sig2 * p[20]) % R
    vkx = bp.g1_mul(g["ic"][0], rho_sum)
    for s, ic in zip(pub_sum, g["ic"][1:]):
        vkx = bp.g1_add(vkx, bp.g1_mul(ic, s))
    g2_sum = bp.g1_add(g2_sum, bp.g1_mul(kz["G_1"], y_sum))
    return pairs + [(bp.g1_mul(g["alpha"], rho_sum), g["beta"]), (vkx, g["gamma"]), (c_sum, g["delta"]), (vk_sum, kz["VK"]), (g2_sum, kz["G_2"])]


def batch_accepts(key, items, scalars):
    """ONE product of this file's Miller values, ONE final exponentiation"""
    f = F12_ONE
    for p1, q2 in batch_pairs(key, items, scalars):
        f = f12_mul(f, miller(q2, p1))
    return bp.final_exponentiate(to_pairing_basis(f)) == bp.F12_ONE
