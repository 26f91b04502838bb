"""The packed-point reference (tests/_point_pack_ref.py) on its own terms, in plain integers: every unpacked point is on its curve, the sign rule holds, both round
trips hold, the Fq2 root agrees with the norm criterion, the bad encodings are refused for the stated reason, and the key packer round-trips over the synthetic
keys of tests/_key_contrib_ref.py.  No GPU, no native code."""
import random

import pytest

from tests import _key_contrib_ref as kref
from tests import _pairing as bp
from tests import _point_pack_ref as ref
from tests._pairing import Q, R


def test_no_y_lists_with_plain_integers():
    for x in ref.G1_NO_Y:
        assert pow(ref.rhs1(x), (Q - 1) // 2, Q) == Q - 1
    for x in ref.G2_NO_Y:
        assert not ref.fq2_is_square(ref.rhs2(x)) and ref.fq2_sqrt(ref.rhs2(x)) is None
    assert pow(3, (Q - 1) // 2, Q) == Q - 1      # 3 is no residue: the Fq2 root of (3, 0) is (0, t)
    assert ref.fq2_sqrt((3, 0))[0] == 0 and ref.fq2_sqrt((4, 0)) in ((2, 0), (Q - 2, 0))


def test_fq_sqrt_agrees_with_euler():
    rng = random.Random("fq_sqrt")
    for a in [0, 1, 3, 4, Q - 1] + [rng.randrange(Q) for _ in range(200)]:
        t = ref.fq_sqrt(a)
        assert (t is not None) == (a == 0 or pow(a, (Q - 1) // 2, Q) == 1)
        assert t is None or t * t % Q == a


def test_fq2_sqrt_agrees_with_the_norm_criterion():
    rng = random.Random("fq2_sqrt")
    vals = ref.sqrt_values() + [(rng.randrange(Q), rng.randrange(Q)) for _ in range(300)]
    squares = 0
    for a in vals:
        r = ref.fq2_sqrt(a)
        assert (r is not None) == ref.fq2_is_square(a), a
        if r is not None:
            assert ref.f2_sqr(r) == a
            squares += 1
    assert 100 < squares < len(vals) - 100      # both kinds were met
    # a1 = 0: every element of Fq is a square in Fq2, through either branch
    for a0 in (4, 3, Q - 4, Q - 3):
        assert ref.f2_sqr(ref.fq2_sqrt((a0, 0))) == (a0, 0)


@pytest.mark.parametrize("group", [1, 2])
def test_points_round_trip_on_the_curve_with_the_sign_rule(group):
    on_curve = bp.g1_on_curve if group == 1 else bp.g2_on_curve
    signs = set()
    for s in ref.scalars(ref.POOL, f"g{group}") + (0,):
        p = ref.point_bytes(group, s)
        packed, f = ref.pack_point_bytes(group, p)
        assert f == 0 and len(packed) == 32 * group
        back, f = ref.unpack_point_bytes(group, packed)
        assert f == 0 and back == p
        assert ref.pack_point_bytes(group, back) == (packed, 0)
        if s == 0:
            assert packed == b"\0" * (32 * group - 1) + b"\x80"
            continue
        pt = kref.g1_at(back, 0) if group == 1 else kref.g2_at(back, 0)
        assert on_curve(pt)
        sign = bool(packed[-1] & 0x40)
        signs.add(sign)
        y = pt[1]
        assert sign == (ref.larger1(y) if group == 1 else ref.larger2(y))
        # the opposite point differs in SIGN alone
        neg = ref.point_bytes(group, R - s)
        assert ref.pack_point_bytes(group, neg)[0] == packed[:-1] + bytes([packed[-1] ^ 0x40])
    assert signs == {False, True}


def test_sign_rule_of_g2_falls_back_to_c0():
    assert ref.larger2((5, 0)) is False and ref.larger2((Q - 5, 0)) is True
    assert ref.larger2((Q - 5, 1)) is False and ref.larger2((5, Q - 1)) is True


@pytest.mark.parametrize("group", [1, 2])
def test_bad_encodings_are_refused_for_the_stated_reason(group):
    for name, (data, finding) in ref.bad_packed(group).items():
        out, f = ref.unpack_point_bytes(group, data)
        assert f == finding and out == b"\0" * (64 * group), name
    for name, (data, finding) in ref.bad_points(group).items():
        out, f = ref.pack_point_bytes(group, data)
        assert f == finding and out == b"\0" * (32 * group), name


@pytest.mark.parametrize("group", [1, 2])
def test_runs_report_the_first_finding(group):
    data = ref.array(group, 9, "first")
    packed, bits, first = ref.run(group, True, data)
    assert (bits, first) == (0, 0) and ref.run(group, False, packed) == (data, 0, 0)
    bad = ref.bad_packed(group)
    a, b = bad["x_is_q"][0], bad["inf_with_sign"][0]
    size = 32 * group
    spoiled = packed[:size * 4] + a + packed[size * 5:size * 7] + b + packed[size * 8:]
    assert ref.run(group, False, spoiled) == (None, ref.COORD, 4)
    assert [f for _, f in ref.per_point(group, False, spoiled)] == [0, 0, 0, 0, ref.COORD, 0, 0, ref.FLAGS, 0]
    assert ref.run(group, True, b"") == (b"", 0, 0)


@pytest.mark.parametrize("shape", [kref.SMALL, kref.LARGE])
@pytest.mark.parametrize("identity", [None, 3])
def test_keys_round_trip(shape, identity):
    key = kref.synthetic_key(kref.DELTA0, shape, identity)
    packed, bits, first = ref.pack_key(key)
    assert bits == 0 and first == (0, 0)
    assert len(packed) == ref.packed_size(len(key)) == 8 * ref.packed_layout(packed)["pwords"]
    assert packed[:8] == b"VG16KPK1" and packed[8:88] == key[8:88]
    assert ref.unpack_key(packed) == (key, 0, (0, 0))
    assert ref.pack_key(ref.unpack_key(packed)[0])[0] == packed
    # the zero slots of b2 (every third) and the identity in l pack as INF alone
    L = ref.packed_layout(packed)
    inf2 = b"\0" * 63 + b"\x80"
    assert all((packed[8 * (L["poff_g2"] + 8 * i):8 * (L["poff_g2"] + 8 * i + 8)] == inf2) == (i % 3 == 2) for i in range(L["n_g2"]))


def test_key_findings_and_refusals():
    key = kref.synthetic_key(kref.DELTA0, kref.SMALL)
    packed = ref.pack_key(key)[0]
    for name, (group, off, poff) in ref.key_point_words(kref.SMALL).items():
        bad = kref.put(key, off + 8 * group - 4, ((kref.coord(key, off + 8 * group - 4) + 1) % Q).to_bytes(32, "little"))      # the last y coordinate + 1
        assert ref.pack_key(bad) == (None, ref.OFF_CURVE, (off, ref.OFF_CURVE)), name
        bad = kref.put(packed, poff + 4 * group - 4, Q.to_bytes(32, "little"))
        assert ref.unpack_key(bad) == (None, ref.COORD, (poff, ref.COORD)), name
    for blob, why in ((packed[:-8], "wrong length"), (packed + b"\0" * 8, "wrong length"), (packed[:1], "not a packed decider key"), (b"", "not a packed decider key"),
                      (key, "not a packed decider key"), (packed[:64], "not a packed decider key")):
        with pytest.raises(ValueError, match=why):
            ref.unpack_key(blob)
    with pytest.raises(ValueError, match="not a decider key"):
        ref.pack_key(packed)
