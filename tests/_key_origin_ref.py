"""Judging that a decider key derives from a powers-of-tau string and a circuit (vimz_decider_key_verify_origin; vimz_amd/csrc/g16_key_origin.hip) stated in plain
Python integers, twice: `verdict` on SCALARS — a point [s]G is its s, as in tests/_g16_powers_ref.py, a pairing equation e([x]G1, [y]G2) = e([u]G1, [v]G2) is
x·y = u·v mod r, and a point that is no known multiple of a generator (off its curve, outside the subgroup, a coordinate not below q) is carried as its finding, which
ends the run before any equation —, and `verify_points` on key BYTES over tests/_pairing.py's points and pairings, for the smallest shapes (a multiplication there takes
40 ms).  tests/test_key_origin_ref_host.py checks the two against each other and against _g16_powers_ref.derive_key and _key_contrib_ref.contribute; the GPU tests
(tests/test_gpu_key_origin.py) take their shapes, tampers and expected words from here.  No GPU, no numpy.  Test infrastructure.

The equations (m wires, n_pub public inputs, n_c constraints, n = 2^logn; P = wires 0..n_pub, Q the rest; rho in (128 bits)^m, rho' in (128 bits)^(n−1)):
    u_X^S = X·rho^S padded to n for X in A, B, C and S in P, Q;  u_A^P[n_c + i] += rho_i for i <= n_pub;  c_X^S = iNTT(u_X^S) with its 1/n;  c_X = c_X^P + c_X^Q
    K(S) = MSM(beta_g1[:n], c_A^S) + MSM(alpha_g1[:n], c_B^S) + MSM(tau_g1[:n], c_C^S)
    a: Σ rho_i·a_i = MSM(tau_g1, c_A)    b1, b2: the same with c_B, in G1 and over tau_g2 in G2    ic: Σ_P rho_i·ic_i = K(P)    l: e(Σ_Q rho_i·l_i, delta2) = e(K(Q), G2)
    h: e(Σ rho'_j·h_j, delta2) = e(MSM(tau_g1[:2n−1], s), G2), s_k = −rho'_k for k < n − 1, + rho'_(k−n) for k >= n      delta: e(delta1, G2) = e(G1, delta2)"""
import functools
import random

from tests import _g16_powers_ref as P
from tests import _g16_ref as G
from tests import _key_contrib_ref as K
from tests import _pairing as bp
from tests._pairing import Q, R
from tests._powers_verify_ref import g2_mul_raw, outside_points

COORD, OFF_CURVE, DELTA, SUBGROUP, HEADER, FIXED_POINTS, A, B1, B2, IC, L, H = (1 << k for k in range(12))      # VIMZ_KEYORIGIN_*
AT_HEADER, AT_FIXED, AT_DELTA, AT_IC, AT_A, AT_B1, AT_L, AT_H, AT_B2 = range(1, 10)                              # VIMZ_KEYORIGIN_AT_*
BIT_NAMES = ("COORD", "OFF_CURVE", "DELTA", "SUBGROUP", "HEADER", "FIXED_POINTS", "A", "B1", "B2", "IC", "L", "H")
ARRAYS = (("ic", AT_IC, 1), ("a", AT_A, 1), ("b1", AT_B1, 1), ("l", AT_L, 1), ("h", AT_H, 1), ("b2", AT_B2, 2))      # in the blob's order: name, place, group
FIXED = ("kzg", "alpha1", "beta1", "beta2", "gamma2")                                                          # first_bad's index for AT_FIXED; groups 2 1 1 2 2
FIXED_GROUP = {"kzg": 2, "alpha1": 1, "beta1": 1, "beta2": 2, "gamma2": 2, "delta1": 1, "delta2": 2}
PP_HASH = 0x0123456789ABCDEF ** 3 % R
TAU, ALPHA, BETA, DELTA0 = 0x2545F4914F6CDD1D0123456789ABCDEF, 0xFEDCBA987654321, 0x55AA55AA55AA77, 0x1B873593CC9E2D51
MAX128 = (1 << 128) - 1


# ---- circuits: a builder's CSRs as they are ---------------------------------------------------------------------------------------------------------------
def spmv(csr, dictionary, v):
    row_ptr, col, coef = csr
    return [sum(dictionary[coef[k]] * v[col[k]] for k in range(row_ptr[r], row_ptr[r + 1])) % R for r in range(len(row_ptr) - 1)]


@functools.lru_cache(maxsize=None)
def circuit(logn, n_pub, n_priv, fill="full", seed=0):
    """a random R1CS: m = 1 + n_pub + n_priv wires, domain 2^logn, n_c = n − n_pub − 1 constraints (fill = "full": the unit rows fill the last slot) or about half
    of that ("half": the tail stays zero), rows of 0..4 terms; the last two wires (when there are four or more private ones) occur in no matrix — their a, b1, b2 and l
    points are the identity —, and B touches few wires, so most of b2 is the identity"""
    rng = random.Random(f"key-origin/{logn}/{n_pub}/{n_priv}/{fill}/{seed}")
    n, m = 1 << logn, 1 + n_pub + n_priv
    n_c = n - n_pub - 1 if fill == "full" else max(1, (n - n_pub - 1) // 2)
    assert n_c >= 1
    dic = [1, R - 1, 2, rng.randrange(1 << 250, R), 0, 3]
    used = m - 2 if n_priv >= 4 else m
    b_wires = sorted(rng.sample(range(used), max(1, used // 3)))
    mats = []
    for q in range(3):
        row_ptr, col, coef = [0], [], []
        for r in range(n_c):
            for _ in range(rng.randrange(5) if r else 2):      # (row 0 is never empty: no matrix is all zero)
                col.append(rng.choice(b_wires) if q == 1 else rng.randrange(used)); coef.append(rng.randrange(len(dic)))
            row_ptr.append(len(col))
        mats.append((row_ptr, col, coef))
    return {"mats": tuple(mats), "dict": dic, "m": m, "n_pub": n_pub, "n_c": n_c, "logn": logn, "n": n, "pp_hash": PP_HASH}


def with_coefficient_changed(circ, q, k=0):
    """the circuit with entry k of matrix q pointing at another coefficient: what a checker holds when the key was made for another circuit"""
    mats = list(circ["mats"])
    row_ptr, col, coef = mats[q]
    coef = list(coef); coef[k] = (coef[k] + 1) % 4      # (among the four non-zero, distinct ones)
    mats[q] = (row_ptr, col, coef)
    return {**circ, "mats": tuple(mats)}


# ---- keys on scalars ------------------------------------------------------------------------------------------------------------------------------------------
def string_of(logn, tau=TAU, alpha=ALPHA, beta=BETA):
    return P.string_scalars(tau, alpha, beta, logn)


def derived_key(circ, string, delta=DELTA0):
    """the key vimz_decider_setup_from_powers derives, on scalars: derive_key's queries and what the blob holds beside them"""
    k = P.derive_key(circ["mats"], circ["dict"], circ["m"], circ["n_pub"], circ["n_c"], circ["logn"], string, delta)
    return {"header": [circ["m"], circ["n_pub"], circ["n_c"], circ["n"], 1, 1], "pp_hash": circ["pp_hash"], "kzg": string["tau_g2"][1], "alpha1": k["alpha"], "beta1": k["beta"],
            "delta1": delta, "beta2": k["beta"], "gamma2": 1, "delta2": delta, "ic": list(k["ic"]), "a": list(k["a"]), "b1": list(k["b"]), "l": list(k["l"]), "h": list(k["h"]),
            "b2": list(k["b"]), "findings": {}}


def contributed(key, delta_p):
    """the key after a contribution of delta' (what _key_contrib_ref.contribute does to the bytes)"""
    dinv = pow(delta_p, -1, R)
    return {**key, "delta1": key["delta1"] * delta_p % R, "delta2": key["delta2"] * delta_p % R, "l": [x * dinv % R for x in key["l"]], "h": [x * dinv % R for x in key["h"]]}


def fixed_rho(circ, label="rho"):
    """(rho, rho') from a seed, with a zero, an all-ones and a small one among them where there is room"""
    rng = random.Random(f"key-origin/rho/{label}/{circ['m']}/{circ['n']}")
    rho, rho_h = [rng.getrandbits(128) for _ in range(circ["m"])], [rng.getrandbits(128) for _ in range(circ["n"] - 1)]
    if circ["m"] >= 6:
        rho[-1], rho[-2] = MAX128, 1
    if circ["n"] >= 8:
        rho_h[1], rho_h[2] = 0, MAX128
    return rho, rho_h


def circuit_side(circ, string, rho, rho_h):
    """the six scalars of the string side: a, b1 (= b2's), K(P), K(Q), the h combination — and the vectors on the way"""
    m, n_pub, n_c, logn, n = circ["m"], circ["n_pub"], circ["n_c"], circ["logn"], circ["n"]
    ninv, winv = pow(n, -1, R), pow(G.omega(logn), -1, R)
    c = {}
    for S, lo, hi in (("P", 0, n_pub + 1), ("Q", n_pub + 1, m)):
        v = [rho[i] if lo <= i < hi else 0 for i in range(m)]
        for X, mat in zip("ABC", circ["mats"]):
            u = spmv(mat, circ["dict"], v) + [0] * (n - n_c)
            if X == "A" and S == "P":
                for i in range(n_pub + 1):
                    u[n_c + i] = (u[n_c + i] + rho[i]) % R
            c[X + S] = [x * ninv % R for x in G.transform(u, winv)]
    t, al, be = string["tau_g1"], string["alpha_g1"], string["beta_g1"]
    dot = lambda base, vec: sum(x * y for x, y in zip(base, vec)) % R      # noqa: E731
    cA, cB = [(x + y) % R for x, y in zip(c["AP"], c["AQ"])], [(x + y) % R for x, y in zip(c["BP"], c["BQ"])]
    Ks = {S: (dot(be, c["A" + S]) + dot(al, c["B" + S]) + dot(t, c["C" + S])) % R for S in "PQ"}
    s = h_scalars(rho_h, n)
    return {"a": dot(t, cA), "b1": dot(t, cB), "b2": dot(string["tau_g2"], cB), "kp": Ks["P"], "kq": Ks["Q"], "h": dot(t[:2 * n - 1], s), "c": c, "s": s}


def h_scalars(rho_h, n):
    return [((rho_h[k - n] if k >= n else 0) - (rho_h[k] if k < n - 1 else 0)) % R for k in range(2 * n - 1)]


def key_side(key, circ, rho, rho_h):
    n_pub = circ["n_pub"]
    dot = lambda pts, w: sum(x * y for x, y in zip(pts, w)) % R      # noqa: E731
    return {"a": dot(key["a"], rho), "b1": dot(key["b1"], rho), "b2": dot(key["b2"], rho), "ic": dot(key["ic"], rho[:n_pub + 1]), "l": dot(key["l"], rho[n_pub + 1:]), "h": dot(key["h"], rho_h)}


def verdict(key, circ, string, rho, rho_h):
    """(bits, (place, index), intermediate scalars or None) of a key on scalars.  key["findings"]: {(array or fixed word's name, index): bit} for the points that are no
    known multiple of the generator."""
    want = [circ["m"], circ["n_pub"], circ["n_c"], circ["n"]]
    for k in range(4):
        if key["header"][k] != want[k]:
            return HEADER, (AT_HEADER, 1 + k), None
    if key["pp_hash"] != circ["pp_hash"]:
        return HEADER, (AT_HEADER, 7 + next(i for i in range(4) if (key["pp_hash"] >> 64 * i) % (1 << 64) != (circ["pp_hash"] >> 64 * i) % (1 << 64))), None
    f = key["findings"]
    for idx, name in enumerate(FIXED + ("delta1", "delta2")):
        if f.get((name, 0)) == COORD:
            return COORD, ((AT_FIXED, idx) if idx < 5 else (AT_DELTA, idx - 5)), None
    fixed_want = {"kzg": string["tau_g2"][1], "alpha1": string["alpha_g1"][0], "beta1": string["beta_g1"][0], "beta2": string["beta_g2"][0], "gamma2": 1}
    for idx, name in enumerate(FIXED):
        if (name, 0) in f or key[name] != fixed_want[name]:
            return FIXED_POINTS, (AT_FIXED, idx), None
    for idx, name in enumerate(("delta1", "delta2")):
        if (name, 0) in f:
            return f[(name, 0)], (AT_DELTA, idx), None
        if key[name] == 0:
            return DELTA, (AT_DELTA, idx), None
    for name, place, _group in ARRAYS:
        found = sorted(i for (a, i) in f if a == name)
        if found:
            bits = 0
            for i in found:
                bits |= f[(name, i)]
            return bits, (place, found[0]), None
    ks, cs = key_side(key, circ, rho, rho_h), circuit_side(circ, string, rho, rho_h)
    bits = 0
    for name, bit, other in (("a", A, "a"), ("b1", B1, "b1"), ("b2", B2, "b2"), ("ic", IC, "kp")):
        if ks[name] != cs[other]:
            bits |= bit
    if ks["l"] * key["delta2"] % R != cs["kq"]:
        bits |= L
    if ks["h"] * key["delta2"] % R != cs["h"]:
        bits |= H
    if key["delta1"] != key["delta2"]:
        bits |= DELTA
    points = [ks["a"], ks["b1"], ks["b2"], ks["ic"], ks["l"], ks["h"], cs["a"], cs["b1"], cs["b2"], cs["kp"], cs["kq"], cs["h"]]
    return bits, (0, 0), points


POINT_GROUPS = (1, 1, 2, 1, 1, 1) * 2      # of verdict's twelve intermediate scalars (b2 on each side is a point of G2; eleven distinct points: both b1 are one scalar's)


# ---- keys as bytes (vimz_decider_key_save's layout) ----------------------------------------------------------------------------------------------------------------
def cpu_points(group, scalars):
    return [K.g1_bytes(bp.g1_mul(bp.G1, s)) if group == 1 else K.g2_bytes(bp.g2_mul(bp.G2, s)) for s in scalars]


def blob_of(key, points=cpu_points, mode=1, len_z=1):
    """the key's bytes; points(group, scalars) -> the points [s]G as bytes (the CPU's, or a GPU test's through vimz_test_g16_fixed_mul)"""
    g1 = points(1, [key["alpha1"], key["beta1"], key["delta1"]] + key["ic"] + key["a"] + key["b1"] + key["l"] + key["h"])
    g2 = points(2, [key["kzg"], key["beta2"], key["gamma2"], key["delta2"]] + key["b2"])
    m, n_pub, n_c, n = key["header"][:4]
    head = b"".join(int(x).to_bytes(8, "little") for x in (K.KEY_MAGIC, m, n_pub, n_c, n, len_z, mode)) + key["pp_hash"].to_bytes(32, "little")
    return head + g2[0] + b"".join(g1[:3]) + b"".join(g2[1:4]) + b"".join(g1[3:]) + b"".join(g2[4:])


def offsets(m, n_pub, n):
    """word offsets of the arrays in a blob"""
    off = {"kzg": 11, "alpha1": 27, "beta1": 35, "delta1": K.KEY_DELTA1, "beta2": 51, "gamma2": 67, "delta2": K.KEY_DELTA2, "ic": K.KEY_IC}
    off["a"] = off["ic"] + 8 * (n_pub + 1); off["b1"] = off["a"] + 8 * m; off["l"] = off["b1"] + 8 * m; off["h"] = off["l"] + 8 * (m - n_pub - 1); off["b2"] = off["h"] + 8 * (n - 1)
    return off


def point_offset(circ, name, index=0):
    group = dict((a, g) for a, _p, g in ARRAYS).get(name) or FIXED_GROUP[name]
    return offsets(circ["m"], circ["n_pub"], circ["n"])[name] + 8 * group * index


# ---- tampers: name -> (key on scalars, what to do to the bytes, the circuit and string the checker holds) ------------------------------------------------------
def tampers(circ, string, delta=DELTA0):
    """name -> {"key": the tampered key on scalars (with its findings), "patch": [(word offset, group, scalar or raw bytes)] to apply to the good key's bytes,
    "circuit", "string": what the checker is given}.  Expected bits and first_bad are verdict's, never written down here."""
    good = derived_key(circ, string, delta)
    m, n_pub, n = circ["m"], circ["n_pub"], circ["n"]
    n_l = m - n_pub - 1
    out = {}

    def put(name, array, index, scalar, key=None):
        k = dict(key or good)
        if array in FIXED_GROUP:
            k[array] = scalar
        else:
            k[array] = list(k[array]); k[array][index] = scalar
        patch = out.get(name, {}).get("patch", []) + [(point_offset(circ, array, index), FIXED_GROUP.get(array) or dict((a, g) for a, _p, g in ARRAYS)[array], scalar)]
        out[name] = {"key": k, "patch": patch, "circuit": circ, "string": string}
        return k

    last = {"ic": n_pub, "a": m - 1, "b1": 0, "l": n_l - 1, "h": n - 2, "b2": 0}
    for array in ("a", "b1", "b2", "ic", "l", "h"):
        i = last[array]
        if array in ("b1", "b2"):      # a wire B touches, so that the point is none of the identities
            i = next(j for j, s in enumerate(good["b1"]) if s)
        put(f"{array}_point_replaced", array, i, (good[array][i] + 12345) % R)
    if m >= 3:      # a_i + T and a_j − T: a combination with equal weights would miss it
        k = put("a_compensating_pair", "a", 0, (good["a"][0] + 777) % R)
        put("a_compensating_pair", "a", m - 1 if m < 6 else 2, (good["a"][m - 1 if m < 6 else 2] - 777) % R, k)
    other = 0x55AA77
    k = dict(good); k["l"] = [x * other % R for x in good["l"]]
    out["l_scaled_by_another_delta"] = {"key": k, "patch": [(point_offset(circ, "l", i), 1, s) for i, s in enumerate(k["l"])], "circuit": circ, "string": string}
    if circ["logn"] >= 2:      # the h query of the domain n/2, padded with identities
        t = string["tau_g1"]; dinv = pow(delta, -1, R); half = n // 2
        k = dict(good); k["h"] = [(t[j + half] - t[j]) * dinv % R for j in range(half - 1)] + [0] * (n - half)
        out["h_of_half_the_domain"] = {"key": k, "patch": [(point_offset(circ, "h", i), 1, s) for i, s in enumerate(k["h"])], "circuit": circ, "string": string}
    for name in FIXED:
        put(f"{name}_swapped", name, 0, (good[name] + 1) % R)
    put("delta1_changed", "delta1", 0, (good["delta1"] + 1) % R)
    for q, X in enumerate("ABC"):
        out[f"circuit_{X}_coefficient"] = {"key": good, "patch": [], "circuit": with_coefficient_changed(circ, q), "string": string}
    # the key of another tau: every query and the KZG point are another string's
    other_string = string_of(circ["logn"], tau=TAU + 2)
    k = derived_key(circ, other_string, delta)
    out["key_of_another_tau"] = {"key": k, "patch": "whole", "circuit": circ, "string": string}
    # the header's m off by one, in a blob that is well formed for it (one more wire, its points the identity): a header that contradicts the blob's length is no key at all
    k = dict(good); k["header"] = [m + 1] + good["header"][1:]
    for array in ("a", "b1", "l", "b2"):
        k[array] = good[array] + [0]
    out["header_m_off_by_one"] = {"key": k, "patch": "whole", "circuit": circ, "string": string}
    # points that are no multiple of a generator: raw bytes, and the finding they carry
    b_i = next(j for j, s in enumerate(good["b2"]) if s)
    mixed = bp.g2_add(bp.g2_mul(bp.G2, good["b2"][b_i]), outside_points()["small"])
    k = dict(good); k["findings"] = {("b2", b_i): SUBGROUP}
    out["b2_point_off_the_subgroup"] = {"key": k, "patch": [(point_offset(circ, "b2", b_i), 2, K.g2_bytes(mixed))], "circuit": circ, "string": string}
    k = dict(good); k["findings"] = {("l", 0): OFF_CURVE}
    out["l_point_off_curve"] = {"key": k, "patch": [(point_offset(circ, "l", 0), 1, K.g1_bytes((5, 5)))], "circuit": circ, "string": string}
    k = dict(good); k["findings"] = {("a", m - 1): COORD}
    out["a_coordinate_is_q"] = {"key": k, "patch": [(point_offset(circ, "a", m - 1), 1, K.g1_bytes((Q, 1)))], "circuit": circ, "string": string}
    return out


REQUIRED_TAMPERS = ("a_point_replaced", "b1_point_replaced", "b2_point_replaced", "ic_point_replaced", "l_point_replaced", "h_point_replaced", "a_compensating_pair",
                    "b2_point_off_the_subgroup", "l_scaled_by_another_delta", "h_of_half_the_domain", "alpha1_swapped", "beta1_swapped", "beta2_swapped", "gamma2_swapped",
                    "kzg_swapped", "delta1_changed", "circuit_A_coefficient", "circuit_B_coefficient", "circuit_C_coefficient", "key_of_another_tau", "header_m_off_by_one")


def apply_patch(blob, tamper, points=cpu_points):
    """the tampered key's bytes from the good key's"""
    if tamper["patch"] == "whole":
        return blob_of(tamper["key"], points)
    for word, group, what in tamper["patch"]:
        blob = K.put(blob, word, what if isinstance(what, bytes) else points(group, [what])[0])
    return blob


# ---- the same verdict on BYTES over tests/_pairing.py (small shapes only) ---------------------------------------------------------------------------------------
def _g1_msm(points, scalars):
    acc = None
    for p, s in zip(points, scalars):
        if p is not None and s % R:
            acc = bp.g1_add(acc, bp.g1_mul(p, s % R))
    return acc


def _g2_msm(points, scalars):
    acc = None
    for p, s in zip(points, scalars):
        if p is not None and s % R:
            acc = bp.g2_add(acc, bp.g2_mul(p, s % R))
    return acc


def verify_points(blob, circ, string_points, rho, rho_h):
    """(bits, (place, index)) of key bytes against a string given as POINTS {"tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2"} (tuples; None never occurs in a
    string), or ValueError with the library's message"""
    lay = K.layout(blob)
    m, n_pub, n = circ["m"], circ["n_pub"], circ["n"]
    words = [int.from_bytes(blob[8 * k:8 * k + 8], "little") for k in range(11)]
    want = [circ["m"], circ["n_pub"], circ["n_c"], circ["n"], None, None] + [(circ["pp_hash"] >> 64 * i) % (1 << 64) for i in range(4)]
    for k in range(10):
        if want[k] is not None and words[1 + k] != want[k]:
            return HEADER, (AT_HEADER, 1 + k)
    if len(string_points["tau_g2"]) < n or len(string_points["tau_g1"]) < 2 * n - 1:
        raise ValueError("the string is shorter than the key's domain: n powers are needed, and 2n - 1 of tau in G1")
    off = offsets(m, n_pub, n)
    assert off["l"] == lay["off_lh"]
    at = lambda name, i=0: K.g1_at(blob, off[name] + 8 * i) if (dict((a, g) for a, _p, g in ARRAYS).get(name) or FIXED_GROUP[name]) == 1 else K.g2_at(blob, off[name] + 16 * i)      # noqa: E731
    flat = lambda p: list(p) if isinstance(p[0], int) else list(p[0]) + list(p[1])      # noqa: E731
    for idx, name in enumerate(FIXED + ("delta1", "delta2")):
        if max(flat(at(name))) >= Q:
            return COORD, ((AT_FIXED, idx) if idx < 5 else (AT_DELTA, idx - 5))
    fixed_want = {"kzg": string_points["tau_g2"][1], "alpha1": string_points["alpha_g1"][0], "beta1": string_points["beta_g1"][0], "beta2": string_points["beta_g2"][0], "gamma2": bp.G2}
    for idx, name in enumerate(FIXED):
        if at(name) != fixed_want[name]:
            return FIXED_POINTS, (AT_FIXED, idx)
    d1, d2 = at("delta1"), at("delta2")
    if not bp.g1_on_curve(d1):
        return OFF_CURVE, (AT_DELTA, 0)
    if K.dec1(d1) is None:
        return DELTA, (AT_DELTA, 0)
    if not bp.g2_on_curve(d2):
        return OFF_CURVE, (AT_DELTA, 1)
    if K.dec2(d2) is None:
        return DELTA, (AT_DELTA, 1)
    if g2_mul_raw(d2, R) is not None:
        return SUBGROUP, (AT_DELTA, 1)
    counts = {"ic": n_pub + 1, "a": m, "b1": m, "l": m - n_pub - 1, "h": n - 1, "b2": m}
    arrays = {}
    for name, place, group in ARRAYS:
        pts, bits, first = [at(name, i) for i in range(counts[name])], 0, None
        for i, p in enumerate(pts):
            if max(flat(p)) >= Q:
                fl = COORD
            elif (K.dec1(p) if group == 1 else K.dec2(p)) is None:
                fl = 0
            elif not (bp.g1_on_curve(p) if group == 1 else bp.g2_on_curve(p)):
                fl = OFF_CURVE
            else:
                fl = SUBGROUP if group == 2 and g2_mul_raw(p, R) is not None else 0
            if fl and first is None:
                first = i
            bits |= fl
        if bits:
            return bits, (place, first)
        arrays[name] = [K.dec1(p) if group == 1 else K.dec2(p) for p in pts]
    # the equations: the circuit side's scalars are the reference's own (circuit_side needs no tau: only c and s are taken from it)
    cs = circuit_side(circ, {"tau_g1": [0] * (2 * n - 1), "tau_g2": [0] * n, "alpha_g1": [0] * n, "beta_g1": [0] * n}, rho, rho_h)
    c = cs["c"]
    t1, t2, al, be = string_points["tau_g1"], string_points["tau_g2"], string_points["alpha_g1"], string_points["beta_g1"]
    cA, cB = [(x + y) % R for x, y in zip(c["AP"], c["AQ"])], [(x + y) % R for x, y in zip(c["BP"], c["BQ"])]
    Ks = {S: bp.g1_add(bp.g1_add(_g1_msm(be, c["A" + S]), _g1_msm(al, c["B" + S])), _g1_msm(t1, c["C" + S])) for S in "PQ"}
    bits = 0
    if _g1_msm(arrays["a"], rho) != _g1_msm(t1, cA):
        bits |= A
    if _g1_msm(arrays["b1"], rho) != _g1_msm(t1, cB):
        bits |= B1
    if _g2_msm(arrays["b2"], rho) != _g2_msm(t2, cB):
        bits |= B2
    if _g1_msm(arrays["ic"], rho[:n_pub + 1]) != Ks["P"]:
        bits |= IC
    one = lambda pairs: bp.pairing_product_is_one([(p, q) for p, q in pairs if p is not None and q is not None])      # noqa: E731
    if not one([(_g1_msm(arrays["l"], rho[n_pub + 1:]), d2), (bp.g1_neg(Ks["Q"]) if Ks["Q"] else None, bp.G2)]):
        bits |= L
    hs = _g1_msm(t1[:2 * n - 1], cs["s"])
    if not one([(_g1_msm(arrays["h"], rho_h), d2), (bp.g1_neg(hs) if hs else None, bp.G2)]):
        bits |= H
    if not one([(d1, bp.G2), (bp.g1_neg(bp.G1), d2)]):
        bits |= DELTA
    return bits, (0, 0)


def string_points_of(string):
    """a string's scalars as points (the CPU's multiplications)"""
    return {"tau_g1": [bp.g1_mul(bp.G1, s) for s in string["tau_g1"]], "alpha_g1": [bp.g1_mul(bp.G1, s) for s in string["alpha_g1"]], "beta_g1": [bp.g1_mul(bp.G1, s) for s in string["beta_g1"]],
            "tau_g2": [bp.g2_mul(bp.G2, s) for s in string["tau_g2"]], "beta_g2": [bp.g2_mul(bp.G2, s) for s in string["beta_g2"]]}


def bit_names(bits):
    return [name for k, name in enumerate(BIT_NAMES) if bits >> k & 1]


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------------------------------------------------------
# (logn, n_pub, private wires, fill): every logn and n_pub the kernels' paths differ at, one private wire and many, full and half-filled domains
DRIVER_SHAPES = ((1, 0, 1, "full"), (3, 2, 1, "half"), (3, 0, 9, "full"), (6, 13, 30, "full"), (7, 2, 70, "half"))
TAMPER_SHAPE = (3, 2, 9, "half")


def spmv_cases():
    """name -> {"mats", "dict", "m", "n_c", "n", "v"} for k_spmv3_dict alone: n_c around a wave and a block; the three paddings (the unit rows' slots are rows like
    the others to this kernel: n − n_c of 1, of several, and n_c = n − 1); rows empty, of 1, 64, 65 and 700 terms; a first, a last and every row empty; a column m − 1;
    a row naming one column twice; coefficients 0, 1, r − 1 and full width; v holding 0, 2^128 − 1 and r − 1; three matrices of different shapes in every call"""
    out = {}
    rng = random.Random("key-origin/spmv")
    dic = [0, 1, R - 1, rng.randrange(1 << 253, R), 2, rng.randrange(1 << 200, 1 << 250)]

    def vec(m):
        v = [rng.randrange(R) for _ in range(m)]
        v[0] = 0
        if m > 2:
            v[1], v[2] = MAX128, R - 1
        v[m - 1] = R - 1 if m > 1 else v[m - 1]
        return v

    def mat(n_c, m, lengths):
        row_ptr, col, coef = [0], [], []
        for r in range(n_c):
            ln = lengths(r)
            cols = [rng.randrange(m) for _ in range(ln)]
            if ln >= 2:
                cols[1] = cols[0]                  # a column named twice
            if ln and r % 3 == 0:
                cols[-1] = m - 1                   # the last column
            col += cols; coef += [rng.randrange(len(dic)) for _ in range(ln)]
            row_ptr.append(len(col))
        return (row_ptr, col, coef)

    for n_c in (1, 63, 64, 65, 257):
        for pad, n in (("tight", n_c + 1), ("loose", 2 * n_c + 7)):
            m = 3 + n_c // 2
            mats = (mat(n_c, m, lambda r: rng.randrange(5)), mat(n_c, m, lambda r: 1), mat(n_c, m, lambda r: 0 if r in (0, n_c - 1) else 3))
            out[f"{n_c}/{pad}"] = {"mats": mats, "dict": dic, "m": m, "n_c": n_c, "n": n, "v": vec(m)}
    long_rows = [0, 1, 64, 65, 700, 0, 2, 63, 700, 1]
    m = 90
    out["long_rows"] = {"mats": (mat(10, m, lambda r: long_rows[r]), mat(10, m, lambda r: long_rows[9 - r]), mat(10, m, lambda r: 0)), "dict": dic, "m": m, "n_c": 10, "n": 16, "v": vec(m)}
    out["n_c_is_n"] = {"mats": (mat(8, 5, lambda r: 2), mat(8, 5, lambda r: 1), mat(8, 5, lambda r: r % 3)), "dict": dic, "m": 5, "n_c": 8, "n": 8, "v": vec(5)}
    return out


def spmv_expected(case):
    return [spmv(M, case["dict"], case["v"]) + [0] * (case["n"] - case["n_c"]) for M in case["mats"]]
