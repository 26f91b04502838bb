"""TEST INFRASTRUCTURE ONLY.  The integer prover of tests/_spartan_ref.py and the independent verifier of tests/_spartan.py for ONE instance with n_pub >= 1
public elements at the LAST n_pub wires of Z (wire 0 stays u) — what vimz_amd/csrc/spartan.hip proves for a CycleFold instance (n_pub = 7) — built from
those modules' pieces: outer_rounds, inner_rounds, ipa_prove, commit; Transcript, Reader, _ipa_verify.  Nothing here reads the library.

What changes with n_pub: the transcript absorbs "X0" .. "X<n_pub-1>" in wire order; comm_W covers wires 1 .. n_w - 1 - n_pub (wire i over ck[i - 1]);
Z(ry) = W'(ry) + u·eq(ry, 0) + sum_k X_k·eq(ry, n_w - n_pub + k); the W opening's b is eq(ry, ·) with wire 0, the public slots and the padding above
the last wire zeroed.  At n_pub = 2 every byte is tests/_spartan_ref.prove_instance's.

FORGERIES (prove(..., forge=index)): a cheating prover that hides a correction under a generator the honest commitment never uses.  For a public slot
(index = n_w - n_pub + k) it claims X_k + 1, commits to comm_W - ck[index - 1] and opens a vector carrying -1 at that index; for a padding slot
(n_w <= index < N) it runs the inner sum-check over a Z with -1 there.  Either convinces a verifier that opens against the UNMASKED eq(ry, ·)
(verify(..., mask=False) shows that these forgeries are real ones) and must be rejected by one that masks.

Host test: tests/test_spartan_pub_ref_host.py; the GPU side: tests/_spartan_pub_gpu.py and tests/test_gpu_spartan_pub.py."""
import functools

import numpy as np

from tests import _spartan_ref as S
from tests._oracle import CURVE_BASE, CURVE_SCALAR, ck_derive, from_limbs, to_limbs
from tests._spartan import Reader, Transcript, _ipa_verify, interp

SHAPES = ((2, 9, 7),        # one committed wire, seven padding slots
          (4, 16, 7),       # n_w a power of two: no padding
          (3, 17, 7),       # the publics straddle index 16, the top variable of ry
          (2, 3, 1),
          (5, 12, 2))       # (n_c, n_w, n_pub)
LABEL = b"vimz-test-spartan-instance-pub"


def case_names():
    return [f"{cid}/{n_c}x{n_w}x{n_pub}/{'relaxed' if rel else 'strict'}" for cid in (0, 1) for n_c, n_w, n_pub in SHAPES for rel in (True, False)]


@functools.lru_cache(maxsize=None)
def case(name):
    """One satisfied instance in the form of _spartan_ref.instance_case, plus "n_pub".  Every public wire occurs in every matrix."""
    cid_s, shape, kind = name.split("/")
    cid, relaxed = int(cid_s), kind == "relaxed"
    n_c, n_w, n_pub = (int(x) for x in shape.split("x"))
    p = S.FIELD[CURVE_SCALAR[cid]]
    rng = S._rng("pub", name)
    nz = lambda: rng.randrange(1, p)      # noqa: E731
    Z = [nz() for _ in range(n_w)]
    if not relaxed:
        Z[0] = 1
    rows = {}
    for m in "ABC":
        rows[m] = [[(rng.randrange(n_w), nz()) for _ in range(rng.randint(1, 3))] for _ in range(n_c)]
        for k in range(n_pub):
            rows[m][k % n_c].append((n_w - n_pub + k, nz()))
    az = [S._dot(t, Z, p) for t in rows["A"]]
    bz = [S._dot(t, Z, p) for t in rows["B"]]
    if relaxed:
        cz = [S._dot(t, Z, p) for t in rows["C"]]
        E = [(x * y - Z[0] * c) % p for x, y, c in zip(az, bz, cz)]
    else:
        E = None
        for r in range(n_c):
            w = rng.randrange(1, n_w - n_pub)
            fix = (az[r] * bz[r] - S._dot(rows["C"][r], Z, p)) * pow(Z[w], -1, p) % p
            if fix:
                rows["C"][r].append((w, fix))
    out = {"cid": cid, "n_w": n_w, "n_c": n_c, "n_pub": n_pub, "Z": Z, "E": E, "digest": rng.randrange(p), "side_tag": (1 if cid == 0 else 2) + (0 if relaxed else 4)}
    for m in "ABC":
        trip = [(r, c, v) for r, terms in enumerate(rows[m]) for c, v in terms]
        rng.shuffle(trip)
        out[m] = trip
    return out


def with_n_pub(c, n_pub=2):
    """a case of _spartan_ref.instance_case as this module takes it"""
    d = dict(c)
    d["n_pub"] = n_pub
    return d


def _neg(P, pb):
    return (0, 0) if tuple(P) == (0, 0) else (P[0], (pb - P[1]) % pb)


def instance_of(orc, c):
    """(cW, cE, u, [X_0 .. X_{n_pub-1}])"""
    cid, n_w, n_pub, Z = c["cid"], c["n_w"], c["n_pub"], c["Z"]
    key = S.key_points(cid)
    cW = S.commit(orc, cid, key[:n_w - 1 - n_pub], Z[1:n_w - n_pub])
    cE = S.commit(orc, cid, key[:c["n_c"]], c["E"]) if c["E"] is not None else (0, 0)
    return cW, cE, Z[0], list(Z[n_w - n_pub:])


def forge_indices(c):
    """every public slot, then one padding slot above the last wire (none when n_w is a power of two)"""
    n_w, n_pub = c["n_w"], c["n_pub"]
    N = 1 << (n_w - 1).bit_length()
    return list(range(n_w - n_pub, n_w)) + ([n_w + (N - n_w) // 2] if N > n_w else [])


def _absorb_instance(tr, c, inst):
    cW, cE, u, X = inst
    tr.absorb(b"side", c["side_tag"].to_bytes(8, "little"))
    tr.fe(b"digest", c["digest"])
    tr.fe(b"cWx", cW[0]); tr.fe(b"cWy", cW[1]); tr.fe(b"cEx", cE[0]); tr.fe(b"cEy", cE[1]); tr.fe(b"u", u)
    for k, x in enumerate(X):
        tr.fe(b"X%d" % k, x)


def prove(orc, c, label=LABEL, forge=None, trace=None):
    """(instance (cW, cE, u, X), the bytes cW ‖ cE ‖ argument).  forge: see the module text.  trace (a dict): receives tau, rx, rho, ry, evalW."""
    cid, n_w, n_c, n_pub, Z, E = c["cid"], c["n_w"], c["n_c"], c["n_pub"], c["Z"], c["E"]
    ps, pb = S.FIELD[CURVE_SCALAR[cid]], S.FIELD[CURVE_BASE[cid]]
    key = S.key_points(cid)
    Ugen = ck_derive(cid, b"vimz-ipa-u", 0)
    s, t = (n_c - 1).bit_length(), (n_w - 1).bit_length()
    Mr, N = 1 << s, 1 << t
    cW, cE, u, X = instance_of(orc, c)
    pad = lambda v, n: list(v) + [0] * (n - len(v))      # noqa: E731
    Zp = pad(Z, N)
    if forge is not None:
        assert n_w - n_pub <= forge < N
        cW = orc.curve_add(cid, cW, _neg(key[forge - 1], pb))
        if forge < n_w:
            X[forge - (n_w - n_pub)] = (X[forge - (n_w - n_pub)] + 1) % ps
        else:
            Zp[forge] = ps - 1
    inst = (cW, cE, u, X)
    out = [S._pt(cW) + S._pt(cE)]
    tr = Transcript(label)
    _absorb_instance(tr, c, inst)
    az, bz, cz = (pad(v, Mr) for v in S.products(c))
    tau = [tr.challenge() for _ in range(s)]
    rx = []

    def outer_challenge(s0, s2, s3):
        out.append(S._fe(s0) + S._fe(s2) + S._fe(s3))
        tr.fe(b"o0", s0); tr.fe(b"o2", s2); tr.fe(b"o3", s3)
        rx.append(tr.challenge())
        return rx[-1]

    _, (_, va, vb, vc, ve) = S.outer_rounds(S.eq_table(tau, ps), az, bz, cz, pad(E, Mr) if E is not None else None, u, outer_challenge, ps)
    for v in (va, vb, vc, ve):
        out.append(S._fe(v))
        tr.fe(b"claim", v)
    rho = tr.challenge()
    ex = S.eq_table(rx, ps)
    mvec = [0] * N
    for m, w in zip("ABC", (1, rho, rho * rho % ps)):
        for r, col, val in c[m]:
            mvec[col] = (mvec[col] + w * ex[r] * val) % ps
    ry = []

    def inner_challenge(s0, s2):
        out.append(S._fe(s0) + S._fe(s2))
        tr.fe(b"i0", s0); tr.fe(b"i2", s2)
        ry.append(tr.challenge())
        return ry[-1]

    _, (_, zr) = S.inner_rounds(mvec, Zp, inner_challenge, ps)
    ey = S.eq_table(ry, ps)
    evalW = (zr - u * ey[0] - sum(x * ey[n_w - n_pub + k] for k, x in enumerate(X))) % ps
    out.append(S._fe(evalW))
    tr.fe(b"evalW", evalW)
    public = lambda i: i == 0 or i + n_pub >= n_w      # noqa: E731  (the padding included)
    Wp = [0 if public(i) else v for i, v in enumerate(pad(Z, N))]
    bW = [0 if public(i) else v for i, v in enumerate(ey)]
    if forge is not None:
        Wp[forge], bW = ps - 1, list(ey)          # (against the whole eq(ry, ·): the opened vector is zero in every other masked slot)
    out.append(S.ipa_prove(orc, cid, tr, Ugen, [key[N - 1]] + key[:N - 1], Wp, bW, cW, evalW, ps))
    if E is not None:
        out.append(S.ipa_prove(orc, cid, tr, Ugen, key[:Mr], pad(E, Mr), ex, cE, ve, ps))
    if trace is not None:
        trace.update(tau=tau, rx=rx, rho=rho, ry=ry, evalW=evalW, claims=(va, vb, vc, ve))
    return inst, b"".join(out)


def spartan_verify(orc, cid, tr, digest, inst, tabs, n_w, n_c, key, Ugen, side_tag, rd, has_E, mask=True):
    """tests/_spartan._spartan_verify for inst = (cW, cE, u, [X...]): None = accepted, else the failed check.  mask=False: the W opening against the whole
    eq(ry, ·) — NOT the protocol; what the forgeries of this module fool."""
    ps, pb = orc.modulus[CURVE_SCALAR[cid]], orc.modulus[CURVE_BASE[cid]]
    cW, cE, u, X = inst
    n_pub = len(X)
    if n_pub < 1 or n_w < n_pub + 2:
        return "shape"
    tr.absorb(b"side", side_tag.to_bytes(8, "little"))
    tr.fe(b"digest", digest)
    tr.fe(b"cWx", cW[0]); tr.fe(b"cWy", cW[1]); tr.fe(b"cEx", cE[0]); tr.fe(b"cEy", cE[1]); tr.fe(b"u", u)
    for k, x in enumerate(X):
        tr.fe(b"X%d" % k, x)
    s, t = (n_c - 1).bit_length(), (n_w - 1).bit_length()
    tau = [tr.challenge() for _ in range(s)]
    claim, rx = 0, []
    for _ in range(s):
        s0, s2, s3 = rd.fe(ps), rd.fe(ps), rd.fe(ps)
        tr.fe(b"o0", s0); tr.fe(b"o2", s2); tr.fe(b"o3", s3)
        r = tr.challenge(); rx.append(r)
        claim = interp([s0, (claim - s0) % ps, s2, s3], r, ps)
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
        r = tr.challenge(); ry.append(r)
        claim = interp([s0, (claim - s0) % ps, s2], r, ps)
    evalW = rd.fe(ps)
    tr.fe(b"evalW", evalW)
    ex, ey = S.eq_table(rx, ps), S.eq_table(ry, ps)
    dic = from_limbs(tabs["dict_canon"])
    vm = 0
    for m, w in zip("ABC", (1, rho, rho * rho % ps)):
        rp, col, coef = tabs[f"{m}_rowptr"], tabs[f"{m}_col"], tabs[f"{m}_coef"]
        acc = 0
        for r in range(len(rp) - 1):
            lo, hi = int(rp[r]), int(rp[r + 1])
            if hi > lo:
                acc += ex[r] * sum(dic[int(coef[k])] * ey[int(col[k])] for k in range(lo, hi))
        vm = (vm + w * acc) % ps
    vz = (evalW + u * ey[0] + sum(x * ey[n_w - n_pub + k] for k, x in enumerate(X))) % ps
    if vm * vz % ps != claim:
        return "inner sum-check"
    N, Mr = 1 << t, 1 << s
    shifted = [key[N - 1]] + list(key[:N - 1])
    eyW = [0 if mask and (i == 0 or i + n_pub >= n_w) else v for i, v in enumerate(ey)]
    if not _ipa_verify(orc, cid, tr, Ugen, np.array(shifted), eyW, cW, evalW, rd, pb, ps):
        return "opening of W"
    if has_E and not _ipa_verify(orc, cid, tr, Ugen, np.array(key[:Mr]), ex, cE, ve, rd, pb, ps):
        return "opening of E"
    return None


@functools.lru_cache(maxsize=None)
def _key_limbs(cid):
    return np.array(to_limbs([co for pt in S.key_points(cid) for co in pt])).reshape(-1, 8)


def verify_bytes(orc, c, blob, inst=None, label=LABEL, mask=True):
    """the verifier above on cW ‖ cE ‖ argument for the instance (u, X) of `c`, or of `inst` (its commitments are read from the blob either way)"""
    cid = c["cid"]
    pb = S.FIELD[CURVE_BASE[cid]]
    rd = Reader(blob)
    try:
        cW, cE = rd.point(pb), rd.point(pb)
        u, X = (c["Z"][0], list(c["Z"][c["n_w"] - c["n_pub"]:])) if inst is None else (inst[2], list(inst[3]))
        why = spartan_verify(orc, cid, Transcript(label), c["digest"], (cW, cE, u, X), S.tables(c), c["n_w"], c["n_c"], _key_limbs(cid),
                             ck_derive(cid, b"vimz-ipa-u", 0), c["side_tag"], rd, c["E"] is not None, mask=mask)
    except ValueError as e:
        return str(e)
    if why is None and rd.pos != len(rd.b):
        return "trailing bytes"
    return why


def inst_words(inst):
    """cW, cE, u, X[...] as the hook vimz_test_spartan_instance_pub_verify takes them: canonical, four words an element"""
    cW, cE, u, X = inst
    return to_limbs([cW[0], cW[1], cE[0], cE[1], u] + list(X))
