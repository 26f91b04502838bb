"""The decider's set-up from a powers-of-tau string (the circuit-specific step of a Groth16 set-up by group operations alone) stated on SCALARS
in plain Python integers — a point [s]G is its s — next to decider_setup_impl's formulas on the trapdoor, and the cases a GPU test of the point kernels (transform,
column sums, same-scalar multiplication; of these the last is built: vimz_amd/csrc/g16_powers.hip, tests/test_gpu_g16_powers_kernels.py) is to run.  No GPU, no numpy.  Checked on the CPU by tests/test_g16_powers_ref_host.py.  Test infrastructure."""
import functools
import random

from tests import _g16_ref as G
from tests._pairing import R

PT_BLOCK = 64                    # threads of a block of k_scale_points, and of the transform's and the column sums' kernels to come
COL_SPLIT = 32                   # a column of more entries is split over workgroups
COL_CHUNK = 1024                 # entries of one workgroup's share of a long column
TRANSFORM_LOGN = {1: (1, 2, 3, 6, 7, 8), 2: (1, 2, 3, 7)}      # n/2 = 32, 64, 128: half a block, one block, two blocks of k_pt_stage; G2: one block edge
COLSUM_COLS = (1, 63, 64, 65)
SCALE_N = (63, 64, 65)


# ---- the string and what the set-up derives from it -----------------------------------------------------------------------------------------
def string_scalars(tau, alpha, beta, power):
    """The scalars of a string of that power: tau_g1 2^(power+1) − 1 powers, tau_g2, alpha_g1, beta_g1 2^power, beta_g2 one."""
    n2 = 1 << power
    pw = [1] * (2 * n2 - 1)
    for k in range(1, len(pw)):
        pw[k] = pw[k - 1] * tau % R
    return {"power": power, "tau_g1": pw, "tau_g2": pw[:n2], "alpha_g1": [alpha * x % R for x in pw[:n2]], "beta_g1": [beta * x % R for x in pw[:n2]], "beta_g2": [beta]}


def lagrange(powers, logn):
    """L_j = 1/n · Σ_k ω^(−jk)·powers[k]: the inverse transform of the first n powers — L_j(tau) when powers[k] = tau^k"""
    n = 1 << logn
    ninv = pow(n, -1, R)
    return [x * ninv % R for x in G.transform(list(powers[:n]), pow(G.omega(logn), -1, R))]


def lagrange_closed_form(tau, logn):
    """L_j(tau) = Z(tau)/n · ω^j / (tau − ω^j), as decider_setup_impl evaluates it"""
    return G.barycentric_weights(tau, logn)


def column_sums(csr, dictionary, n_cols, values):
    """Q_j = Σ_{r, k: col[k] = j} dict[coef[k]]·values[r] for a CSR (row_ptr, col, coef)"""
    row_ptr, col, coef = csr
    out = [0] * n_cols
    for r in range(len(row_ptr) - 1):
        for k in range(row_ptr[r], row_ptr[r + 1]):
            out[col[k]] = (out[col[k]] + dictionary[coef[k]] * values[r]) % R
    return out


def derive_key(mats, dictionary, m, n_pub, n_c, logn, string, delta):
    """The key's scalars as the set-up derives them from a string's scalars: a, b (both groups), ic, l, h, and the verifying points' alpha, beta, gamma = 1, delta"""
    n = 1 << logn
    assert (1 << string["power"]) >= n and len(string["tau_g1"]) >= 2 * n - 1
    L, aL, bL = lagrange(string["tau_g1"], logn), lagrange(string["alpha_g1"], logn), lagrange(string["beta_g1"], logn)
    a = column_sums(mats[0], dictionary, m, L)
    for i in range(n_pub + 1):
        a[i] = (a[i] + L[n_c + i]) % R
    b = column_sums(mats[1], dictionary, m, L)
    k = [(x + y + z) % R for x, y, z in zip(column_sums(mats[0], dictionary, m, bL), column_sums(mats[1], dictionary, m, aL), column_sums(mats[2], dictionary, m, L))]
    for i in range(n_pub + 1):                              # (the rows of the constant and the public inputs belong to A: beta times them is in K)
        k[i] = (k[i] + bL[n_c + i]) % R
    dinv = pow(delta, -1, R)
    t = string["tau_g1"]
    return {"a": a, "b": b, "ic": k[:n_pub + 1], "l": [x * dinv % R for x in k[n_pub + 1:]], "h": [(t[j + n] - t[j]) * dinv % R for j in range(n - 1)],
            "alpha": string["alpha_g1"][0], "beta": string["beta_g1"][0], "gamma": 1, "delta": delta}


def trapdoor_key(mats, dictionary, m, n_pub, n_c, logn, tau, alpha, beta, gamma, delta):
    """The same key by decider_setup_impl's formulas on the trapdoor: the QAP evaluated at tau through the closed form of the Lagrange basis"""
    n = 1 << logn
    L = lagrange_closed_form(tau, logn)
    u, v, w = (column_sums(M, dictionary, m, L) for M in mats)
    for i in range(n_pub + 1):
        u[i] = (u[i] + L[n_c + i]) % R
    k = [(beta * x + alpha * y + z) % R for x, y, z in zip(u, v, w)]
    ginv, dinv = pow(gamma, -1, R), pow(delta, -1, R)
    z_tau = (pow(tau, n, R) - 1) % R
    return {"a": u, "b": v, "ic": [x * ginv % R for x in k[:n_pub + 1]], "l": [x * dinv % R for x in k[n_pub + 1:]],
            "h": [z_tau * dinv % R * pow(tau, j, R) % R for j in range(n - 1)], "alpha": alpha, "beta": beta, "gamma": gamma, "delta": delta}


# ---- cases of the kernel tests --------------------------------------------------------------------------------------------------------------------
def _rng(*what):
    return random.Random("g16-powers/" + "/".join(str(x) for x in what))


@functools.lru_cache(maxsize=None)
def transform_cases(logn):
    """name -> the scalars s_k of the input points [s_k]G; 0 is the identity"""
    n, rng = 1 << logn, _rng("transform", logn)
    rnd = [rng.randrange(1, R) for _ in range(n)]
    holes = list(rnd)
    for k in rng.sample(range(n), max(1, n // 4)):
        holes[k] = 0
    half = rnd[:n // 2] + rnd[:n // 2]                      # P_k = P_{k + n/2}: the last stage's butterflies with twiddle one double
    c = rng.randrange(1, R)
    return {"random": rnd, "e_0": [1] + [0] * (n - 1), "e_1": [0, 1] + [0] * (n - 2), "constant": [c] * n, "identity": [0] * n, "holes": holes, "half_period": half}


FULL_CASES = ("random", "holes")          # these run every direction; the other vectors the forward transform alone (a launch costs one scalar multiplication's latency)


def transform_expected(v, logn, name="random"):
    """what the runs of a case give: forward; and for FULL_CASES inverse unscaled, inverse, and both inverses of the forward"""
    n, w = 1 << logn, G.omega(logn)
    if name not in FULL_CASES:
        return {"fwd": G.transform(v, w)}
    winv, ninv = pow(w, -1, R), pow(n, -1, R)
    inv = G.transform(v, winv)
    return {"fwd": G.transform(v, w), "inv": inv, "inv_scaled": [x * ninv % R for x in inv], "back_unscaled": [x * n % R for x in v], "back": list(v)}


def coefficients():
    """1, r − 1, 2, 2^k, r − 2^k, full-size random, 0"""
    rng = _rng("coefficients")
    return [1, R - 1, 2, 1 << 17, 1 << 200, R - (1 << 17), R - (1 << 200), 3, R - 3] + [rng.randrange(1 << 250, R) for _ in range(4)] + [(R + 1) // 2, (R - 1) // 2, 0]


@functools.lru_cache(maxsize=None)
def colsum_case(n_cols, variant="mixed"):
    """-> dict(n_rows, n_cols, csr = (row_ptr, col, coef), dict, scalars of the rows' points).  Rows 0..: random points; some rows share a point, some hold the
    opposite of another's, some the identity.  Column lengths: `variant` = an int: every column that many entries; "empty": no entries at all; "mixed": columns
    of COL_SPLIT − 1, COL_SPLIT, COL_SPLIT + 1, 0, 1, COL_CHUNK + 1, COL_CHUNK entries, a doubling pair, a cancelling pair, a cancelling pair followed by a third
    point, the rest 0..5 entries."""
    rng = _rng("colsum", n_cols, variant)
    n_rows = COL_CHUNK + 76
    s = [rng.randrange(1, R) for _ in range(n_rows)]
    for r in range(8, n_rows, 97):
        s[r] = 0                                            # identity points
    s[1] = s[0]                                             # rows 0, 1 share a point; row 2 holds its opposite
    s[2] = R - s[0]
    dic = coefficients()
    per_col = [[] for _ in range(n_cols)]                    # column -> [(row, coefficient index)]

    cheap = [i for i, c in enumerate(dic) if min(c, R - c) < 4]      # a full-size coefficient costs 254 doublings in its thread: one entry in eight

    def fill(j, count):
        if j < n_cols:
            per_col[j] = [(r, rng.randrange(len(dic)) if rng.randrange(8) == 0 else rng.choice(cheap)) for r in sorted(rng.sample(range(n_rows), count))]

    if variant == "empty":
        pass
    elif isinstance(variant, int):
        for j in range(n_cols):
            fill(j, variant)
    else:
        for j, count in enumerate([COL_SPLIT - 1, COL_SPLIT, COL_SPLIT + 1, 0, 1, COL_CHUNK + 1, COL_CHUNK]):
            fill(j, count)
        special = {7: [(0, 0), (1, 0)], 8: [(0, 0), (2, 0)], 9: [(0, 0), (2, 0), (5, 0)], 10: [(0, 2), (2, 2), (5, 12)], 11: [(0, 0), (0, 0), (0, 0)]}
        for j, ent in special.items():
            if j < n_cols:
                per_col[j] = ent
        for j in range(12, n_cols):
            fill(j, rng.randrange(6))
    rows = [[] for _ in range(n_rows)]
    for j, ent in enumerate(per_col):
        for r, c in ent:
            rows[r].append((j, c))
    row_ptr, col, coef = [0], [], []
    for r in range(n_rows):
        for j, c in rows[r]:
            col.append(j); coef.append(c)
        row_ptr.append(len(col))
    return {"n_rows": n_rows, "n_cols": n_cols, "csr": (row_ptr, col, coef), "dict": dic, "scalars": s}


def colsum_cases():
    out = {f"{n}/mixed": (n, "mixed") for n in COLSUM_COLS}
    out.update({f"1/{k}": (1, k) for k in (0, 1, COL_SPLIT - 1, COL_SPLIT, COL_SPLIT + 1)})
    out["64/empty"] = (64, "empty")
    return out


def colsum_expected(case):
    return column_sums(case["csr"], case["dict"], case["n_cols"], case["scalars"])


@functools.lru_cache(maxsize=None)
def scale_points(n):
    rng = _rng("scale", n)
    s = [rng.randrange(1, R) for _ in range(n)]
    s[0] = 0
    s[n // 2] = 0
    return s


def scale_scalars():
    return {"one": 1, "two": 2, "minus_one": R - 1, "random": _rng("scale/scalar").randrange(1 << 250, R)}
