"""The reference the GPU test of the k-public-element argument compares against (tests/_spartan_pub_ref.py), validated on the CPU: at n_pub = 2 against the
prover and the verifier it generalises, byte for byte; at n_pub = 1 and 7 against the definitions by brute force; and its forgeries against a verifier that does
not mask the public and padding slots (they fool it: they are real forgeries) and one that does (they are rejected).  No GPU."""
import pytest

from tests import _oracle
from tests import _spartan_pub_ref as P
from tests import _spartan_ref as S


@pytest.fixture(scope="module")
def orc():
    return _oracle.load()


@pytest.mark.parametrize("name", S.instance_names())
def test_two_publics_give_the_bytes_of_the_reference_it_generalises(orc, name):
    base = S.instance_case(name)
    c = P.with_n_pub(base, 2)
    want = S.prove_instance(orc, base)
    inst, blob = P.prove(orc, c, label=S.LABEL)
    assert blob == want
    assert inst == (S.instance_of(orc, base)[0], S.instance_of(orc, base)[1], base["Z"][0], list(base["Z"][-2:]))
    # the two verifiers agree: on the honest bytes, on X0 + 1 and on a flipped bit in each place
    assert P.verify_bytes(orc, c, blob, label=S.LABEL) is None and S.verify_bytes(orc, base, blob) is None
    ps = S.FIELD[_oracle.CURVE_SCALAR[c["cid"]]]
    bumped = (None, None, inst[2], [(inst[3][0] + 1) % ps, inst[3][1]])
    assert P.verify_bytes(orc, c, blob, inst=bumped, label=S.LABEL) == S.verify_bytes(orc, base, blob, X0_delta=1) != None      # noqa: E711
    for what, off in S.argument_layout(base).items():
        bad = S.flip(blob, 128 + off)
        assert P.verify_bytes(orc, c, bad, label=S.LABEL) == S.verify_bytes(orc, base, bad) != None, what      # noqa: E711


def _eq(pt, idx, p):
    """eq(pt, idx) by the product formula, pt[0] the top bit"""
    k, acc = len(pt), 1
    for q, r in enumerate(pt):
        acc = acc * (r if (idx >> (k - 1 - q)) & 1 else 1 - r) % p
    return acc


def _mle(v, pt, p):
    return sum(x * _eq(pt, i, p) for i, x in enumerate(v)) % p


@pytest.mark.parametrize("name", [n for n in P.case_names() if n.split("/")[1].split("x")[2] in ("1", "7")])
def test_one_and_seven_publics_against_brute_force(orc, name):
    c = P.case(name)
    cid, n_w, n_c, n_pub, Z = c["cid"], c["n_w"], c["n_c"], c["n_pub"], c["Z"]
    p = S.FIELD[_oracle.CURVE_SCALAR[cid]]
    az, bz, cz = S.products(c)
    e = c["E"] if c["E"] is not None else [0] * n_c
    assert all((x * y - Z[0] * w - v) % p == 0 for x, y, w, v in zip(az, bz, cz, e))          # the case is satisfied
    for m in "ABC":
        assert set(range(n_w - n_pub, n_w)) <= {col for _, col, _ in c[m]}                  # every public wire is used
    tr = {}
    inst, blob = P.prove(orc, c, trace=tr)
    cW, cE, u, X = inst
    assert u == Z[0] and X == Z[n_w - n_pub:] and len(X) == n_pub
    # the commitment covers wires 1 .. n_w - 1 - n_pub, wire i over ck[i - 1]
    key = S.key_points(cid)
    acc = (0, 0)
    for i in range(1, n_w - n_pub):
        acc = orc.curve_add(cid, acc, orc.curve_mul(cid, key[i - 1], Z[i]))
    assert tuple(acc) == tuple(cW)
    s, t = (n_c - 1).bit_length(), (n_w - 1).bit_length()
    assert len(blob) == 128 + S.argument_size(c)                                              # (the counts do not depend on n_pub)
    # the outer claims are the multilinear extensions of Az, Bz, Cz, E at rx; the first round's polynomial sums to zero over {0, 1}
    va, vb, vc, ve = tr["claims"]
    assert (va, vb, vc, ve) == tuple(_mle(v, tr["rx"], p) for v in (az, bz, cz, e))
    rd = P.Reader(blob[128:])
    s0, s2, s3 = rd.fe(), rd.fe(), rd.fe()
    tab = [_eq(tr["tau"], i, p) for i in range(1 << s)]
    pad = lambda v, n: list(v) + [0] * (n - len(v))      # noqa: E731
    A_, B_, C_, E_ = (pad(v, 1 << s) for v in (az, bz, cz, e))
    half = (1 << s) // 2
    assert s0 == sum(tab[i] * (A_[i] * B_[i] - u * C_[i] - E_[i]) for i in range(half)) % p
    assert (s0 + sum(tab[i] * (A_[i] * B_[i] - u * C_[i] - E_[i]) for i in range(half, 2 * half))) % p == 0
    # evalW is the extension of the committed part alone, and adding the public entries' share gives Z(ry)
    ry = tr["ry"]
    assert len(ry) == t
    evalW = sum(Z[i] * _eq(ry, i, p) for i in range(1, n_w - n_pub)) % p
    assert tr["evalW"] == evalW
    assert (evalW + u * _eq(ry, 0, p) + sum(X[k] * _eq(ry, n_w - n_pub + k, p) for k in range(n_pub))) % p == _mle(Z, ry, p)
    assert P.verify_bytes(orc, c, blob) is None
    assert P.prove(orc, c)[1] == blob


@pytest.mark.parametrize("name", P.case_names())
def test_verifier_binds_every_public_element(orc, name):
    c = P.case(name)
    p = S.FIELD[_oracle.CURVE_SCALAR[c["cid"]]]
    inst, blob = P.prove(orc, c)
    assert P.verify_bytes(orc, c, blob) is None
    for k in range(c["n_pub"]):
        X = list(inst[3]); X[k] = (X[k] + 1) % p
        assert P.verify_bytes(orc, c, blob, inst=(None, None, inst[2], X)) is not None, f"X{k} + 1 accepted"
    assert P.verify_bytes(orc, c, blob, inst=(None, None, (inst[2] + 1) % p, inst[3])) is not None, "u + 1 accepted"
    for what, off in S.argument_layout(c).items():
        assert P.verify_bytes(orc, c, S.flip(blob, 128 + off)) is not None, what


@pytest.mark.parametrize("name", P.case_names())
def test_forgeries_fool_an_unmasked_verifier_only(orc, name):
    c = P.case(name)
    n_w, n_pub = c["n_w"], c["n_pub"]
    idx = P.forge_indices(c)
    assert idx[:n_pub] == list(range(n_w - n_pub, n_w)) and len(idx) == n_pub + (0 if n_w & (n_w - 1) == 0 else 1)
    honest, _ = P.prove(orc, c)
    for i in idx:
        inst, blob = P.prove(orc, c, forge=i)
        assert inst[0] != honest[0] and (inst[3] != honest[3]) == (i < n_w)
        assert P.verify_bytes(orc, c, blob, inst=inst, mask=False) is None, f"slot {i}: not a forgery"
        assert P.verify_bytes(orc, c, blob, inst=inst) == "opening of W", f"slot {i}: accepted"
