"""The decider's NTT, quotient, fixed-base and G2 multi-scalar kernels (vimz_amd/csrc/groth16.hip) restated in plain Python integers, and the
cases tests/test_gpu_g16_kernels.py runs them on.  No GPU, no numpy.  The references check each other in tests/test_g16_ref_host.py before they
judge a kernel; the group arithmetic is tests/_pairing.py's, pinned by the pairing tests.  Test infrastructure."""
import functools
import random

from tests._pairing import G2, Q, R, g2_add, g2_mul

GEN = 5                          # generates Fr's multiplicative group: the roots of unity and the coset are its powers
DFT_MAX_LOGN = 8                 # up to here the transforms are the O(n²) definition; above, ntt (checked against it up to here)
TRANSFORM_LOGN = (1, 2, 3, 8, 9, 10, 13)      # n/2 = 128, 256: half a block and one block of k_ntt_stage; 13: 16 blocks per stage
FIXED_N = (1, 127, 128, 129)     # k_fixed_mul's block is 128 threads
MSM_N = (1, 63, 64, 65, 2047, 2048, 2049, 4160)      # around a wave and around G2_PLANE_THREADS = 2048; 4160 = 65 waves' worth
MSM_EDGE_N = (65, 2049, 4160)
MSM_POOL = 4160


def omega(logn):
    return pow(GEN, (R - 1) >> logn, R)


# ---- transforms ---------------------------------------------------------------------------------------------------------------------------
def dft(v, w):
    """out[i] = Σ_j v[j]·w^(i j): the definition."""
    n = len(v)
    pw = [1] * n
    for k in range(1, n):
        pw[k] = pw[k - 1] * w % R
    return [sum(x * pw[i * j % n] for j, x in enumerate(v)) % R for i in range(n)]


def ntt(v, w):
    """The same sums by the radix-2 recursion over even and odd positions."""
    n = len(v)
    if n == 1:
        return list(v)
    w2 = w * w % R
    ev, od = ntt(v[0::2], w2), ntt(v[1::2], w2)
    out, t, h = [0] * n, 1, n // 2
    for k in range(h):
        x = t * od[k] % R
        out[k], out[k + h] = (ev[k] + x) % R, (ev[k] - x) % R
        t = t * w % R
    return out


def transform(v, w):
    return dft(v, w) if len(v) <= 1 << DFT_MAX_LOGN else ntt(v, w)


def coset_extend(v, logn):
    """Evaluations over H = <ω> -> evaluations over 5·H: interpolate, scale coefficient i by 5^i, evaluate."""
    n, w = 1 << logn, omega(logn)
    ninv = pow(n, -1, R)
    coef = [x * ninv % R for x in transform(v, pow(w, -1, R))]
    return transform([c * pow(GEN, i, R) % R for i, c in enumerate(coef)], w)


def quotient_pipeline(a, b, c, logn):
    """The prover's sequence step by step: h = (A·B − C) / Z evaluated on the coset, where Z = 5^n − 1 is constant, then brought back to coefficients."""
    n, w = 1 << logn, omega(logn)
    ea, eb, ec = (coset_extend(v, logn) for v in (a, b, c))
    zinv = pow(pow(GEN, n, R) - 1, -1, R)
    q = [(x * y - z) * zinv % R for x, y, z in zip(ea, eb, ec)]
    ninv, ginv = pow(n, -1, R), pow(GEN, -1, R)
    coef = transform(q, pow(w, -1, R))
    return [x * ninv % R * pow(ginv, i, R) % R for i, x in enumerate(coef)]


def interpolate(v, logn):
    """Coefficients of the polynomial of degree < n with v as its values over H, by the O(n²) inverse DFT."""
    n = 1 << logn
    ninv = pow(n, -1, R)
    return [x * ninv % R for x in dft(v, pow(omega(logn), -1, R))]


def quotient_schoolbook(a, b, c, logn):
    """Without the coset: A·B − C coefficient by coefficient is h·(X^n − 1) = X^n·h − h for satisfied inputs — the low half is minus the high half."""
    n = 1 << logn
    A, B, C = (interpolate(v, logn) for v in (a, b, c))
    prod = [0] * (2 * n)
    for i, x in enumerate(A):
        if x:
            for j, y in enumerate(B):
                prod[i + j] = (prod[i + j] + x * y) % R
    for i, z in enumerate(C):
        prod[i] = (prod[i] - z) % R
    low, high = prod[:n], prod[n:]
    assert all((x + y) % R == 0 for x, y in zip(low, high)), "A·B − C is no multiple of X^n − 1: the inputs are not satisfied"
    return high


def barycentric_weights(x, logn):
    """u_i with f(x) = Σ u_i·f(ω^i) for every f of degree < n: (x^n − 1)/n · ω^i / (x − ω^i).  x outside H."""
    n, w = 1 << logn, omega(logn)
    c = (pow(x, n, R) - 1) * pow(n, -1, R) % R
    out, t = [], 1
    for _ in range(n):
        out.append(c * t % R * pow((x - t) % R, -1, R) % R)
        t = t * w % R
    return out


def dot(u, v):
    return sum(x * y for x, y in zip(u, v)) % R


def horner(coef, x):
    acc = 0
    for c in reversed(coef):
        acc = (acc * x + c) % R
    return acc


def quotient_identity_holds(a, b, c, h, logn, x):
    """A(x)·B(x) − C(x) == h(x)·(x^n − 1) at one point outside H."""
    u = barycentric_weights(x, logn)
    return (dot(u, a) * dot(u, b) - dot(u, c) - horner(h, x) * (pow(x, 1 << logn, R) - 1)) % R == 0


def identity_points(logn):
    rng = random.Random(f"g16/points/{logn}")
    return [rng.randrange(2, R) for _ in range(2)]


# ---- cases: transforms and quotients ----------------------------------------------------------------------------------------------------------
def unit(n, k):
    return [1 if i == k else 0 for i in range(n)]


def transform_cases(logn):
    """name -> vector.  The unit vectors' transforms are rows of the DFT matrix: twiddle order and bit reversal element by element."""
    n = 1 << logn
    rng = random.Random(f"g16/transform/{logn}")
    return {"random": [rng.randrange(R) for _ in range(n)], "max": [R - 1] * n, "zero": [0] * n, "constant": [rng.randrange(1, R)] * n,
            "e_0": unit(n, 0), "e_1": unit(n, 1), "e_half": unit(n, n // 2), "e_last": unit(n, n - 1)}


def quotient_cases(logn):
    """name -> (a, b, c, satisfied)."""
    n, w = 1 << logn, omega(logn)
    rng = random.Random(f"g16/quotient/{logn}")
    had = lambda a, b: [x * y % R for x, y in zip(a, b)]      # noqa: E731
    out = {}
    a, b = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
    out["random"] = (a, b, had(a, b), True)
    top = [pow(w, i * (n - 1), R) for i in range(n)]          # A = B = X^(n−1): h = X^(n−2), the highest coefficient a quotient can have
    out["top_degree"] = (top, top, had(top, top), True)
    ka, kb = [rng.randrange(1, R)] * n, [rng.randrange(1, R)] * n
    out["constant"] = (ka, kb, had(ka, kb), True)             # h = 0
    out["a_zero"] = ([0] * n, b, [0] * n, True)
    mx, mb = [R - 1] * n, [R - 1 if i % 2 == 0 else rng.randrange(R) for i in range(n)]
    out["max"] = (mx, mb, had(mx, mb), True)
    c = had(a, b)
    c[3 % n] = (c[3 % n] + 1) % R                             # c = a∘b + e_3: no polynomial quotient — the pipeline's words all the same (− c and zinv)
    out["unsatisfied"] = (a, b, c, False)
    return out


# ---- cases: fixed-base multiplication -----------------------------------------------------------------------------------------------------------
def fixed_special_scalars():
    s = [0, 1, 2, 15, 16, 17]
    s += [1 << (4 * w) for w in range(64)]                    # one digit 1 in every window; 2^252 is the top window's
    s += [15 << (4 * w) for w in (0, 1, 7, 8, 31, 62)]        # the largest digit, at word boundaries (w = 7, 8) too
    s += [3 << 252]                                           # the top window's largest digit: r >> 252 == 3
    s += [R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
    s += [int("0f" * 32, 16) % R, int("11" * 32, 16) % R]
    return s


def fixed_scalars(n):
    """The scalars of one call: the special ones first, random ones after them up to n (n = 1: one random scalar — 0 alone would be no multiplication)."""
    rng = random.Random("g16/fixed")
    full = fixed_special_scalars()
    full += [rng.randrange(R) for _ in range(max(FIXED_N) - len(full))]
    assert len(full) == max(FIXED_N) >= n
    return [full[-1]] if n == 1 else full[:n]


# ---- cases: the G2 multi-scalar multiplication ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def msm_pool_scalars():
    """k_i of the bases k_i·G2 (made on the GPU by the fixed-base hook, checked there against g2_mul)."""
    rng = random.Random("g16/msm/pool")
    return tuple(rng.randrange(1, R) for _ in range(MSM_POOL))


@functools.lru_cache(maxsize=None)
def msm_cases():
    """name -> {"bases": [b_i], "scalars": [s_i], "form": 0 canonical / 1 Montgomery}.  b_i = j + 1: the pool's point j; −(j + 1): its negative; 0: the identity."""
    out = {}
    seq = lambda n: list(range(1, n + 1))      # noqa: E731
    for n in MSM_N:
        rng = random.Random(f"g16/msm/random/{n}")
        out[f"random/{n}"] = {"bases": seq(n), "scalars": [rng.randrange(R) for _ in range(n)], "form": 1}
    out["random_canonical/65"] = dict(out["random/65"], form=0)
    for n in MSM_EDGE_N:
        rng = random.Random(f"g16/msm/edge/{n}")
        kinds = {"max": [R - 1] * n,                                       # full planes: the queue holds exactly 64 every round
                 "one": [1] * n, "zero": [0] * n,
                 "top_plane": [1 << 253] * n,                              # plane 253 alone
                 "lane0_off": [0 if i % 64 == 0 else 1 for i in range(n)],      # 63 of 64 lanes: the queue's remainder walks 63, 62, …
                 "density": [sum((rng.random() < (i % 64) / 64) << j for j in range(253)) for i in range(n)]}      # lane l's bits are set with probability l/64
        for k, s in kinds.items():
            out[f"{k}/{n}"] = {"bases": seq(n), "scalars": s, "form": 1}
    n = MSM_POOL
    rng = random.Random("g16/msm/special")
    same = [1] * n                                                         # every lane adds P to P: the doubling branch of add_mixed; 4160·P
    signs = [1] * 2048 + [-1] * 2048 + [1] * (n - 4096)                    # every lane cancels to the identity, lanes of wave 0 start again; 64·P
    t = rng.randrange(2, R)
    out["same_base"] = {"bases": same, "scalars": [1] * n, "form": 1}
    out["cancel_restart"] = {"bases": signs, "scalars": [1] * n, "form": 1}
    out["identity_every_tenth"] = {"bases": [0 if i % 10 == 0 else i + 1 for i in range(n)], "scalars": [1] * n, "form": 1}
    out["same_base_scaled"] = {"bases": same, "scalars": [t] * n, "form": 1}
    out["cancel_restart_scaled"] = {"bases": signs, "scalars": [t] * n, "form": 1}
    # opposite and equal operands where the patterns above do not put them: between the threads of k_g2_plane_tree (threads 0..31 hold P, 64..95 −P: the first fold
    # cancels them; 96..127 hold Q, folded by doublings to 32·Q) and in the host's Horner (plane 1 = P, plane 0 = ∓2P: 2·P − 2P and 2·P + 2P)
    out["tree_cancel"] = {"bases": [1] * 32 + [0] * 32 + [-1] * 32 + [2] * 32, "scalars": [1] * 128, "form": 1}
    out["horner_cancel"] = {"bases": [1, -1, -1], "scalars": [2, 1, 1], "form": 1}
    out["horner_double"] = {"bases": [1, 1, 1], "scalars": [2, 1, 1], "form": 1}
    return out


MSM_REPEAT = "random/2049"       # run twice on one context


def msm_layout(case):
    """The hook's wire vector and wire numbers for a case: m = 2n + 3 wires, wire 2i + 1 holds s_i, the others are random and must not be read."""
    n = len(case["scalars"])
    rng = random.Random(f"g16/msm/wires/{n}")
    wires = [rng.randrange(R) for _ in range(2 * n + 3)]
    idx = [2 * i + 1 for i in range(n)]
    for i, s in zip(idx, case["scalars"]):
        wires[i] = s
    return wires, idx


def msm_multiplier(case, pool_k):
    """Σ s_i·k_i mod r with k_i the multiplier of base i: the sum is this multiple of the generator."""
    k = lambda b: 0 if b == 0 else pool_k[b - 1] if b > 0 else -pool_k[-b - 1]      # noqa: E731
    return sum(s * k(b) for s, b in zip(case["scalars"], case["bases"])) % R


def g2_neg(p):
    return None if p is None else (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q))


def msm_explicit(case, pool_pts):
    """The same sum point by point (small n)."""
    acc = None
    for s, b in zip(case["scalars"], case["bases"]):
        p = None if b == 0 else pool_pts[b - 1] if b > 0 else g2_neg(pool_pts[-b - 1])
        acc = g2_add(acc, g2_mul(p, s)) if p is not None else acc
    return acc


def g2_words(p):
    """A point as the hooks write it: x.c0, x.c1, y.c0, y.c1; the identity as zeros."""
    return [0, 0, 0, 0] if p is None else [p[0][0], p[0][1], p[1][0], p[1][1]]


def g2_from_words(w):
    return None if not any(w) else ((w[0], w[1]), (w[2], w[3]))


def g2_gen_mul(k):
    return g2_mul(G2, k)
