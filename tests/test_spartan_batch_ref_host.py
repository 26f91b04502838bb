"""tests/_spartan_batch_ref.py — the batched compressed-proof verifier in Python integers — tied to what exists, on the CPU: the unrolled group equation of every
opening against the integer provers and the independent verifier of tests/_spartan_ref.py and tests/_spartan_pub_ref.py, the closed form of an E opening's dot, the
index map of a W opening, and the batch equation under random multipliers.  No GPU."""
import random

import pytest

from tests import _oracle
from tests import _spartan_batch_ref as B
from tests import _spartan_pub_ref as P
from tests import _spartan_ref as S
from tests._oracle import CURVE_SCALAR


@pytest.fixture(scope="module")
def orc():
    return _oracle.load()


ALL_CASES = S.instance_names() + P.case_names()


@pytest.mark.parametrize("name", ALL_CASES)
def test_the_unrolled_equation_holds_for_every_opening(orc, name):
    c, label, blob = B.proof_of(orc, name)
    d = B.deferred_bytes(c, blob, label)
    assert isinstance(d, dict), d
    ps = S.FIELD[CURVE_SCALAR[c["cid"]]]
    assert not d["trailing"]
    assert len(d["openings"]) == (2 if c["E"] is not None else 1)
    assert B.mat_eval(c, d["rx"], d["ry"], d["w"], ps) * d["vz"] % ps == d["claim"]
    for op in d["openings"]:
        assert len(op["Q"]) == len(op["c"]) == 2 * op["rounds"] + 1
        assert B.opening_holds(orc, c["cid"], op), f"{name}: {'W' if op['shifted'] else 'E'} opening"
    assert B.verify_bytes(orc, c, blob, label) is None


@pytest.mark.parametrize("name", S.instance_names())
def test_tampered_bytes_fail_the_unrolled_equation_iff_the_verifier_refuses(orc, name):
    """test_spartan_ref_host's tamper cases: a flipped bit at each place of argument_layout, and X0 + 1"""
    c, label, blob = B.proof_of(orc, name)
    ps = S.FIELD[CURVE_SCALAR[c["cid"]]]
    for what, off in S.argument_layout(c).items():
        bad = S.flip(blob, 128 + off)
        want = S.verify_bytes(orc, c, bad)
        got = B.verify_bytes(orc, c, bad, label)
        assert (want is None) == (got is None), f"{name}: flipped bit in the {what}: the verifier says {want!r}, the unrolled equation {got!r}"
        assert want is not None
    u, X = B.case_inst(c)
    X1 = [(X[0] + 1) % ps] + X[1:]
    assert S.verify_bytes(orc, c, blob, X0_delta=1) is not None and B.verify_bytes(orc, c, blob, label, X=X1) is not None
    assert (S.verify_bytes(orc, c, blob) is None) and (B.verify_bytes(orc, c, blob, label) is None)


@pytest.mark.parametrize("name", P.case_names())
def test_public_elements_and_u_bind_the_deferred_verifier(orc, name):
    c, label, blob = B.proof_of(orc, name)
    ps = S.FIELD[CURVE_SCALAR[c["cid"]]]
    u, X = B.case_inst(c)
    assert B.verify_bytes(orc, c, blob, label, u=(u + 1) % ps) is not None
    for k in range(len(X)):
        Xb = list(X); Xb[k] = (Xb[k] + 1) % ps
        assert B.verify_bytes(orc, c, blob, label, X=Xb) is not None
        assert P.verify_bytes(orc, c, blob, inst=(None, None, u, Xb)) is not None


@pytest.mark.parametrize("fid", (0, 1))
def test_the_dot_of_an_e_opening_has_a_closed_form(fid):
    p = S.FIELD[fid]
    rng = random.Random(f"batch-dot/{fid}")
    for rounds in (1, 2, 5, 9):
        xs, pt = [rng.getrandbits(128) for _ in range(rounds)], [rng.randrange(p) for _ in range(rounds)]
        assert B.masked_dot(xs, pt, 0, 0, p) == B.dot_closed_form(xs, pt, p)
    xs, pt = [0, p - 1, 5], [p - 1, 0, 7]
    assert B.masked_dot(xs, pt, 0, 0, p) == B.dot_closed_form(xs, pt, p)


def test_the_s_vector_and_its_index_map():
    p = S.FIELD[0]
    xs = [3, 5, 7]                              # round 0 = the top bit
    assert B.svec(xs, p) == [1, 7, 5, 35, 3, 21, 15, 105]
    assert [B.slot_of(i, 8, True) for i in range(8)] == [7, 0, 1, 2, 3, 4, 5, 6]          # index 0 on ck[n − 1], index i on ck[i − 1]
    assert [B.slot_of(i, 8, False) for i in range(8)] == list(range(8))
    # the masked dot leaves out index 0, the public tail and the padding
    pt = [11, 13, 17]
    b = S.eq_table(pt, p)
    s = B.svec(xs, p)
    assert B.masked_dot(xs, pt, 2, 7, p) == sum(s[i] * b[i] for i in (1, 2, 3, 4)) % p
    acc = B.accumulators([{"rounds": 3, "xs": xs, "afin": 2, "shifted": True}, {"rounds": 2, "xs": [3, 5], "afin": 1, "shifted": False}], [1, 10], 8, p)
    assert acc == [2 * 7 + 10, 2 * 5 + 50, 2 * 35 + 30, 2 * 3 + 150, 2 * 21, 2 * 15, 2 * 105, 2 * 1]


def test_unrolled_coefficients_are_the_round_by_round_update():
    """P <- R + x·P + x²·L over scalars standing in for points"""
    p = S.FIELD[1]
    rng = random.Random("batch-unroll")
    for rounds in (1, 2, 6):
        xs = [rng.getrandbits(128) for _ in range(rounds)]
        comm, claim, r0, U = (rng.randrange(p) for _ in range(4))
        Ls, Rs = [rng.randrange(p) for _ in range(rounds)], [rng.randrange(p) for _ in range(rounds)]
        Pt = (comm + claim * r0 * U) % p
        for x, L, R in zip(xs, Ls, Rs):
            Pt = (R + x * Pt + x * x * L) % p
        c0, cR, cL, g0 = B.unroll(xs, claim, r0, p)
        assert (c0 * comm + sum(a * b for a, b in zip(cR, Rs)) + sum(a * b for a, b in zip(cL, Ls)) + g0 * U) % p == Pt


@pytest.mark.parametrize("cid", (0, 1))
def test_a_batch_with_one_wrong_final_scalar_is_refused_and_accepted_without_it(orc, cid):
    names = [f"{cid}/8x8/relaxed", f"{cid}/9x5/strict", f"{cid}/5x33/relaxed", f"{cid}/8x8/strict"]
    ops, owner = [], []
    for k, name in enumerate(names):
        c, label, blob = B.proof_of(orc, name)
        if k == 3:
            blob = B.bump_final_scalar(c, blob)
            assert S.verify_bytes(orc, c, blob) == "opening of W"
        d = B.deferred_bytes(c, blob, label)
        assert isinstance(d, dict)          # (afin + 1 passes every scalar check: only the group equation sees it)
        ops += d["openings"]; owner += [k] * len(d["openings"])
    rng = random.Random(f"batch-multipliers/{cid}")
    rhos = [rng.getrandbits(128) | 1 for _ in ops]
    big = 64
    assert not B.batch_holds(orc, cid, ops, rhos, big)[0]
    keep = [i for i, k in enumerate(owner) if k != 3]
    assert B.batch_holds(orc, cid, [ops[i] for i in keep], [rhos[i] for i in keep], big)[0]
    assert B.batch_holds(orc, cid, [ops[i] for i in keep], [1] * len(keep), big)[0]
