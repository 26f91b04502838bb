"""The multilinear KZG opening (vimz_mlkzg_open / vimz_mlkzg_verify; vimz_amd/csrc/mlkzg.hip, mlkzg_verify.hpp) restated on plain Python integers: the
prover with a KNOWN tau — a commitment is then [P(tau)]G, one g1_mul, so any ℓ is cheap —, the stages of its kernels (fold, evaluation at r, −r, r², batching, the
chunked division with its carries) and the verifier over tests/_pairing.py.  Statements and proofs cross this file as lists of u64 words, the layout of the C ABI:
an element is 4 little-endian words, a G1 point x then y with the identity as zeros, [tau]G2 as x.c0, x.c1, y.c0, y.c1.  Test infrastructure only: nothing of the
product imports this."""
import hashlib

from tests._pairing import G1, G2, Q, R, g1_add, g1_mul, g1_neg, g1_on_curve, g2_mul, g2_on_curve, pairing_product_is_one

MALFORMED, OFF_CURVE, FOLD, PAIRING = 1, 2, 4, 8      # VIMZ_MLKZG_*
MAX_LOGN = 26
M64 = (1 << 64) - 1


def words_of(x):
    return [(x >> (64 * k)) & M64 for k in range(4)]


def int_of(w):
    return sum(int(w[k]) << (64 * k) for k in range(4))


def point_words(p):
    return [0] * 8 if p is None else words_of(p[0]) + words_of(p[1])


def point_of(w):
    x, y = int_of(w[:4]), int_of(w[4:8])
    return None if x == 0 and y == 0 else (x, y)


def g2_words(p):
    return words_of(p[0][0]) + words_of(p[0][1]) + words_of(p[1][0]) + words_of(p[1][1])


def vk_words(tau):
    return g2_words(g2_mul(G2, tau))


def proof_words(logn):
    return 20 * logn + 16


class Transcript:
    """the SHA3-256 chain of vimz_amd/csrc/proof_io.hpp"""

    def __init__(self, label):
        self.st = bytes(32)
        self.absorb(b"init", label)

    def absorb(self, tag, data):
        self.st = hashlib.sha3_256(self.st + tag[:8].ljust(8, b"\0") + len(data).to_bytes(8, "little") + data).digest()

    def absorb_words(self, tag, w):
        self.absorb(tag, b"".join(int(x).to_bytes(8, "little") for x in w))

    def challenge(self):
        self.st = hashlib.sha3_256(self.st + b"c").digest()
        return int.from_bytes(self.st[:16], "little")


def challenges(logn, comm_w, point_w, eval_w, proof):
    """(r, q, d) from the statement's and the proof's words"""
    t = Transcript(b"vimz-mlkzg-v1")
    t.absorb_words(b"logn", [logn]); t.absorb_words(b"C", comm_w); t.absorb_words(b"x", point_w); t.absorb_words(b"y", eval_w)
    t.absorb_words(b"Ck", proof[:8 * (logn - 1)])
    r = t.challenge()
    t.absorb_words(b"E", proof[8 * (logn - 1):8 * (logn - 1) + 12 * logn])
    q = t.challenge()
    t.absorb_words(b"W", proof[8 * (logn - 1) + 12 * logn:])
    return r, q, t.challenge()


# ---- the stages ---------------------------------------------------------------------------------------------------------------------------------------------------
def mle_eval(v, x):
    """y by its definition: Σ_i v[i]·Π_k (bit_k(i) ? x_k : 1 − x_k), bit_k the k-th LOWEST bit of i"""
    y = 0
    for i, c in enumerate(v):
        e = c
        for k, xk in enumerate(x):
            e = e * (xk if (i >> k) & 1 else 1 - xk) % R
        y = (y + e) % R
    return y


def fold_levels(v, x):
    """P_0 .. P_ℓ for v already padded to 2^ℓ"""
    P = [list(v)]
    for xk in x:
        p = P[-1]
        P.append([(p[2 * j] + xk * (p[2 * j + 1] - p[2 * j])) % R for j in range(len(p) // 2)])
    return P


def horner(p, u):
    a = 0
    for c in reversed(p):
        a = (a * u + c) % R
    return a


def eval3(p, r):
    return [horner(p, r), horner(p, -r % R), horner(p, r * r % R)]


def batch_levels(levels, q):
    """B[j] = Σ_{k: j < len(P_k)} q^k·P_k[j] over the levels given (the last, single-element level P_ℓ is not among them)"""
    out = [0] * len(levels[0])
    for k, p in enumerate(levels):
        qk = pow(q, k, R)
        for j, c in enumerate(p):
            out[j] = (out[j] + qk * c) % R
    return out


def divide(b, u):
    """(quotient of len(b) − 1 coefficients, remainder) of b by (X − u), by the recurrence q_(i−1) = b_i + u·q_i"""
    quot, carry = [0] * (len(b) - 1), 0
    for i in range(len(b) - 1, -1, -1):
        carry = (b[i] + u * carry) % R
        if i:
            quot[i - 1] = carry
    return quot, carry


def division_carries(b, u, chunk):
    """what the first two launches of the division leave: each chunk's carry-out with a zero carry-in, and the carry INTO each chunk"""
    n = -(-len(b) // chunk)
    out = [horner(b[chunk * t:chunk * (t + 1)], u) for t in range(n)]
    cin, acc, uc = [0] * n, 0, pow(u, chunk, R)
    for t in range(n - 1, -1, -1):
        cin[t] = acc
        acc = (out[t] + uc * acc) % R
    return out, cin


def commit(tau, p):
    return g1_mul(G1, horner(p, tau))


# ---- prover and verifier ------------------------------------------------------------------------------------------------------------------------------------------
def prove(tau, v, logn, x):
    """The opening of v (1 <= len(v) <= 2^logn) at x under the SRS of tau: {"comm", "eval", "proof": words, and what the prover went through}"""
    N = 1 << logn
    assert 1 <= len(v) <= N and len(x) == logn
    P = fold_levels(list(v) + [0] * (N - len(v)), x)
    y = P[logn][0]
    comm = point_words(commit(tau, P[0]))
    proof = [w for k in range(1, logn) for w in point_words(commit(tau, P[k]))]
    point_w = [w for xk in x for w in words_of(xk)]
    r, _, _ = challenges(logn, comm, point_w, words_of(y), proof + [0] * (proof_words(logn) - len(proof)))
    if r == 0:
        raise ValueError("the challenge r is zero")
    us = [r, -r % R, r * r % R]
    E = [[horner(P[k], u) for k in range(logn)] for u in us]
    proof += [w for row in E for e in row for w in words_of(e)]
    _, q, _ = challenges(logn, comm, point_w, words_of(y), proof + [0] * 24)
    B = batch_levels(P[:logn], q)
    quots, rems = [], []
    for j, u in enumerate(us):
        quot, rem = divide(B, u)
        assert rem == horner(E[j], q), "the remainder rule"
        quots.append(quot); rems.append(rem)
        proof += point_words(commit(tau, quot))
    assert len(proof) == proof_words(logn)
    r2, q2, d = challenges(logn, comm, point_w, words_of(y), proof)
    assert (r2, q2) == (r, q)
    return {"comm": comm, "eval": y, "proof": proof, "point_words": point_w, "levels": P, "r": r, "q": q, "d": d, "E": E, "B": B, "quotients": quots, "remainders": rems}


def parse(vk_w, comm_w, logn, point_w, eval_w, proof):
    """the range checks: None when malformed"""
    if not 1 <= logn <= MAX_LOGN or len(proof) != proof_words(logn) or len(point_w) != 4 * logn:
        return None
    el = [int_of(point_w[4 * k:4 * k + 4]) for k in range(logn)] + [int_of(eval_w)]
    a, b = 8 * (logn - 1), 8 * (logn - 1) + 12 * logn
    E = [int_of(proof[a + 4 * i:a + 4 * i + 4]) for i in range(3 * logn)]
    coords = [int_of(w[4 * i:4 * i + 4]) for w in (vk_w, comm_w, proof[:a], proof[b:]) for i in range(len(w) // 4)]
    if any(e >= R for e in el + E) or any(c >= Q for c in coords):
        return None
    vk = ((int_of(vk_w[0:4]), int_of(vk_w[4:8])), (int_of(vk_w[8:12]), int_of(vk_w[12:16])))
    return {"vk": vk, "C": point_of(comm_w), "x": el[:logn], "y": el[logn], "ck": [point_of(proof[8 * k:8 * k + 8]) for k in range(logn - 1)],
            "E": [E[u * logn:(u + 1) * logn] for u in range(3)], "W": [point_of(proof[b + 8 * u:b + 8 * u + 8]) for u in range(3)]}


def fold_equations(x, y, E, r):
    """for every k whether 2r·next_k = r(1 − x_k)(E_r[k] + E_(−r)[k]) + x_k(E_r[k] − E_(−r)[k]) holds"""
    logn = len(x)
    out = []
    for k in range(logn):
        nxt = E[2][k + 1] if k + 1 < logn else y
        out.append(2 * r * nxt % R == (r * (1 - x[k]) * (E[0][k] + E[1][k]) + x[k] * (E[0][k] - E[1][k])) % R)
    return out


def pairing_sides(P, r, q, d):
    """(L, Rr) with the equation e(L, G2) = e(Rr, [tau]G2)"""
    Cs = [P["C"]] + P["ck"]
    cb = None
    for k, c in enumerate(Cs):
        cb = g1_add(cb, g1_mul(c, pow(q, k, R)))
    us = [r, -r % R, r * r % R]
    L = Rr = None
    for j, u in enumerate(us):
        dj = pow(d, j, R)
        term = g1_add(g1_add(cb, g1_neg(g1_mul(G1, horner(P["E"][j], q)))), g1_mul(P["W"][j], u))
        L = g1_add(L, g1_mul(term, dj))
        Rr = g1_add(Rr, g1_mul(P["W"][j], dj))
    return L, Rr


def verify(vk_w, comm_w, logn, point_w, eval_w, proof):
    """the verdict word of vimz_mlkzg_verify"""
    P = parse(vk_w, comm_w, logn, point_w, eval_w, proof)
    if P is None:
        return MALFORMED
    if not all(g1_on_curve(p) for p in [P["C"]] + P["ck"] + P["W"]) or not g2_on_curve(P["vk"]) or g2_mul(P["vk"], R) is not None:
        return OFF_CURVE
    r, q, d = challenges(logn, comm_w, point_w, eval_w, proof)
    if r == 0 or not all(fold_equations(P["x"], P["y"], P["E"], r)):
        return FOLD
    L, Rr = pairing_sides(P, r, q, d)
    pairs = [(p, g) for p, g in ((L, G2), (g1_neg(Rr), P["vk"])) if p is not None]
    return 0 if pairing_product_is_one(pairs) else PAIRING
