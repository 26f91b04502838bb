"""The commitment-opening chains of the full decider's check 5 (vimz_amd/csrc/aug/decider_cf.hpp) in plain Python integers, and the cases the host test
(tests/test_cf_chains_ref_host.py) and the GPU test (tests/test_gpu_decider_chains.py) both run.  Test infrastructure.

Grumpkin: y² = x³ − 17 over BN254's scalar field (P below); its group has BN254's base-field prime Q points.  A scalar s < Q over generator G_k walks 127
two-bit windows from H: window j adds the table entry (d + 1)·4^j·G_k for the digit d = bit(2j) + 2·bit(2j + 1) by an affine addition; its four wires
are (b0·b1, slope, x, y).  The chain ends at H + (s + Σ_j 4^j)·G_k."""
import functools
import random

P = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001      # coordinates (BN254 Fr)
Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47      # scalars (BN254 Fq): the group's order
B = -17
G = (1, 17631683881184975370165255887551781615748388533673675138860)
WINDOWS = 127
OFFSET = sum(4 ** j for j in range(WINDOWS))      # what the "+ 1" of every window's digit adds to the scalar

assert (G[1] * G[1] - (G[0] ** 3 + B)) % P == 0


def on_curve(p):
    return (p[1] * p[1] - (p[0] ** 3 + B)) % P == 0


def batch_inv(xs):
    """inverses modulo P of a list of non-zero residues, one modular inversion in all"""
    pre, run = [], 1
    for x in xs:
        pre.append(run); run = run * x % P
    inv = pow(run, -1, P)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % P; inv = inv * xs[i] % P
    return out


def batch_add(ps, qs):
    """p + q for lists of affine points with different x, and the slopes"""
    lam = [(q[1] - p[1]) * i % P for p, q, i in zip(ps, qs, batch_inv([(q[0] - p[0]) % P for p, q in zip(ps, qs)]))]
    out = []
    for p, q, l in zip(ps, qs, lam):
        x = (l * l - p[0] - q[0]) % P
        out.append((x, (l * (p[0] - x) - p[1]) % P))
    return out, lam


def batch_dbl(ps):
    lam = [3 * p[0] * p[0] * i % P for p, i in zip(ps, batch_inv([2 * p[1] % P for p in ps]))]
    out = []
    for p, l in zip(ps, lam):
        x = (l * l - 2 * p[0]) % P
        out.append((x, (l * (p[0] - x) - p[1]) % P))
    return out


# ---- an independent scalar multiplication: Jacobian double-and-add, the identity as None -----------------------------------------------------------
def _jdbl(p):
    X, Y, Z = p
    if Y == 0:
        return None
    S = 4 * X * Y * Y % P; M = 3 * X * X % P
    X3 = (M * M - 2 * S) % P
    return X3, (M * (S - X3) - 8 * pow(Y, 4, P)) % P, 2 * Y * Z % P


def _jadd_affine(p, q):
    if p is None:
        return q[0], q[1], 1
    X, Y, Z = p
    Z2 = Z * Z % P
    U2, S2 = q[0] * Z2 % P, q[1] * Z2 * Z % P
    if U2 == X:
        return _jdbl(p) if S2 == Y else None
    H_, R_ = (U2 - X) % P, (S2 - Y) % P
    H2 = H_ * H_ % P; H3 = H2 * H_ % P
    X3 = (R_ * R_ - H3 - 2 * X * H2) % P
    return X3, (R_ * (X * H2 - X3) - Y * H3) % P, Z * H_ % P


def mul(p, k):
    """k·p (affine; None = the identity)"""
    acc = None
    for i in range(k.bit_length() - 1, -1, -1):
        if acc is not None:
            acc = _jdbl(acc)
        if (k >> i) & 1:
            acc = _jadd_affine(acc, p)
    if acc is None:
        return None
    zi = pow(acc[2], -1, P)
    return acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P


def add(p, q):
    """p + q for affine points (None = the identity)"""
    if p is None:
        return q
    r = _jadd_affine((p[0], p[1], 1), q)
    if r is None:
        return None
    zi = pow(r[2], -1, P)
    return r[0] * zi * zi % P, r[1] * zi * zi * zi % P


def neg(p):
    return p[0], (P - p[1]) % P


@functools.lru_cache(maxsize=None)
def multiples(n):
    """G_k = (k + 1)·G for k < n"""
    out = [G, batch_dbl([G])[0]]
    while len(out) < n:
        out.append(batch_add([out[-1]], [G])[0][0])
    return tuple(out[:n])


# ---- the table and the chains -------------------------------------------------------------------------------------------------------------------
def table(gens):
    """T[k][j][d] = (d + 1)·4^j·G_k, window by window over all the generators at once"""
    n = len(gens)
    T = [[None] * WINDOWS for _ in range(n)]
    base = list(gens)
    for j in range(WINDOWS):
        p2 = batch_dbl(base)
        p3, _ = batch_add(p2, base)
        p4 = batch_dbl(p2)
        for k in range(n):
            T[k][j] = (base[k], p2[k], p3[k], p4[k])
        base = p4
    return T


def digits(s):
    return [(s >> (2 * j)) & 3 for j in range(WINDOWS)]


def chains(T, H, scalars):
    """(wires [k][j] = (b0·b1, slope, x, y), end points [k], bad): scalar k over generator k.  bad: an addition met two points with the same x — nothing
    more is computed then (wires and ends None)."""
    cnt = len(scalars)
    dg = [digits(s) for s in scalars]
    acc = [H] * cnt
    wires = [[None] * WINDOWS for _ in range(cnt)]
    for j in range(WINDOWS):
        qs = [T[k][j][dg[k][j]] for k in range(cnt)]
        if any(q[0] == a[0] for q, a in zip(qs, acc)):
            return None, None, True
        acc, lam = batch_add(acc, qs)
        for k in range(cnt):
            wires[k][j] = (1 if dg[k][j] == 3 else 0, lam[k], acc[k][0], acc[k][1])
    return wires, acc, False


def rows_hold(H, Tk, s, wk):
    """the three rows of add_incomplete per window, and the product row of its two bits, for one scalar's wires"""
    acc = H
    for j, (pr, lam, x, y) in enumerate(wk):
        b0, b1 = (s >> (2 * j)) & 1, (s >> (2 * j + 1)) & 1
        q = Tk[j][b0 + 2 * b1]
        if pr != b0 * b1:
            return False
        if ((q[0] - acc[0]) * lam - (q[1] - acc[1])) % P or (lam * lam - (x + acc[0] + q[0])) % P or ((acc[0] - x) * lam - (y + acc[1])) % P:
            return False
        acc = (x, y)
    return True


def flat(wires, ends):
    """the integers in the order vimz_test_decider_chains writes them: wires_out, ends_out"""
    return [v for wk in wires for w in wk for v in w], [c for e in ends for c in e]


# ---- the cases -----------------------------------------------------------------
SIZES = (1, 63, 64, 65, 257)      # a wave's edge, a workgroup's edge (one wave per workgroup), past them
CYCLE = sum(((j % 4) << (2 * j)) for j in range(WINDOWS))      # digits 0, 1, 2, 3, 0, ... (the top window's digit is 126 % 4 = 2: bit 253 alone of the top two, below q)
SPECIAL = {
    "zero": 0,                              # every digit 0
    "one": 1,
    "all_bits": ((1 << 254) - 1) % Q,       # 2^254 − 1 reduced below q
    "q_minus_1": Q - 1,                     # the top window's digit is 3
    "cycle": CYCLE % Q,
    "bit_253": 1 << 253,
    "bit_252": 1 << 252,
}
assert all(0 <= s < Q for s in SPECIAL.values()) and digits(Q - 1)[WINDOWS - 1] == 3 and digits(0) == [0] * WINDOWS and digits(CYCLE)[:8] == [0, 1, 2, 3, 0, 1, 2, 3]


def _random_scalars(tag, n):
    rng = random.Random(f"cf-chains/{tag}")
    return [rng.randrange(Q) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (n_gens, scalars): generators G_k = (k + 1)·G, scalar k over generator k"""
    out = {}
    for name, s in SPECIAL.items():
        out[f"1/{name}"] = (1, [s])
    out["1/random"] = (1, _random_scalars("1", 1))
    out["63/same_random"] = (63, _random_scalars("63", 1) * 63)
    out["64/different"] = (64, list(SPECIAL.values()) + _random_scalars("64", 64 - len(SPECIAL)))
    out["65/different"] = (65, _random_scalars("65", 65 - len(SPECIAL)) + list(SPECIAL.values()))
    out["65/same_q_minus_1"] = (65, [Q - 1] * 65)
    out["257/different"] = (257, list(SPECIAL.values()) + _random_scalars("257", 257 - len(SPECIAL)))
    out["257/same_cycle"] = (257, [SPECIAL["cycle"]] * 257)
    return out


DEGENERATE = ("G0_is_H", "G0_is_minus_H")      # inside a launch of 65 chains: scalar 0 over G_0 = ±H meets H in window 0


def degenerate_case(name, H):
    """(generators as points, scalars): 65 chains, the first one 0 over G_0 = H (a doubling) or −H (the sum is the identity); the others honest"""
    gens = list(multiples(65))
    gens[0] = H if name == "G0_is_H" else neg(H)
    return gens, [0] + _random_scalars(name, 64)


@functools.lru_cache(maxsize=None)
def shared_table():
    """the table of G_0 .. G_256, once per process"""
    return table(multiples(max(SIZES)))


def expected(name, H):
    """(wires, ends) of a case of cases() as flat lists of integers"""
    n, sc = cases()[name]
    w, e, bad = chains(shared_table(), H, sc)
    assert not bad
    return flat(w, e)


# ---- vimz_test_decider_chains (include/vimz_hip_testing.h) ---------------------------------------------------------------------------------------------
def _words(vals):
    import numpy as np
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").astype(np.uint64)


def _ints(arr):
    raw = arr.tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def run_hook(lib, ctx_handle, where, gens, scalars):
    """the hook over generators (affine points) and scalars: (rc, wires, ends, H, bad) — wires and ends as flat lists of integers"""
    import ctypes as C
    import numpy as np
    vp = C.c_void_p
    lib.vimz_test_decider_chains.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, C.POINTER(C.c_int)]
    lib.vimz_test_decider_chains.restype = C.c_int
    g = _words([c for p in gens for c in p]); s = _words(scalars)
    cnt = len(scalars)
    wires = np.full(cnt * WINDOWS * 4 * 4, 7, dtype=np.uint64); ends = np.full(cnt * 8, 7, dtype=np.uint64); h = np.zeros(8, dtype=np.uint64)
    bad = C.c_int(-1)
    rc = lib.vimz_test_decider_chains(ctx_handle, where, g.ctypes.data_as(vp), len(gens), s.ctypes.data_as(vp), cnt, wires.ctypes.data_as(vp),
                                      ends.ctypes.data_as(vp), h.ctypes.data_as(vp), C.byref(bad))
    return rc, _ints(wires), _ints(ends), tuple(_ints(h)), bad.value
