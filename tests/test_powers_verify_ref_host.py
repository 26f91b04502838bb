"""tests/_powers_verify_ref.py against itself and tests/_pairing.py: the verdict vimz_powers_verify gives, stated in plain Python.  What the GPU tests and the CPU
loop of the kernels' functions take from it must be right before they compare against it: the square root in Fq2, the points outside the subgroup (and that a
reduced scalar multiplication would not notice them), the verdict on a good string and on strings with one thing wrong, the combination cut into chunks."""
import random

import pytest

from tests import _g16_powers_ref as W
from tests import _pairing as bp
from tests import _powers_verify_ref as V
from tests._pairing import Q, R

TAU, ALPHA, BETA, POWER = 0x1234567890ABCDEF1234567, 0xFEDCBA987654321, 0x55AA55AA55AA77, 2


@pytest.fixture(scope="module")
def good():
    return V.string_points(W.string_scalars(TAU, ALPHA, BETA, POWER))


@pytest.fixture(scope="module")
def rho(good):
    rng = random.Random("powers_verify/rho")
    return [rng.getrandbits(128) for _ in range(len(good["tau_g1"]) - 1)]


def test_the_square_root_in_fq2():
    rng = random.Random("f2_sqrt")
    for _ in range(8):
        a = (rng.randrange(Q), rng.randrange(Q))
        sq = bp._f2_mul(a, a)
        root = V.f2_sqrt(sq)
        assert root is not None and bp._f2_mul(root, root) == sq
    assert V.f2_sqrt((0, 0)) == (0, 0) and V.f2_sqrt((Q - 1, 0)) in ((0, 1), (0, Q - 1))
    non_squares = [a for a in ((k, 1) for k in range(2, 12)) if V.f2_sqrt(a) is None]
    assert non_squares                                                        # half of Fq2 has no root: some of ten do not
    for a in non_squares:
        assert V.f2_pow(a, (Q * Q - 1) // 2) == (Q - 1, 0)                    # Euler's criterion agrees


def test_the_points_outside_the_subgroup():
    assert V.COFACTOR % V.SMALL_FACTORS[0] == 0 and V.COFACTOR % V.SMALL_FACTORS[1] == 0
    out = V.outside_points()
    for name, p in out.items():
        assert bp.g2_on_curve(p) and V.g2_mul_raw(p, R) is not None, name
        assert V.point_flags(2, p) == V.SUBGROUP
    for x in ((2, 0), (2, 1), (3, 1)):
        p = V.twist_point(x)
        assert p is not None and bp.g2_on_curve(p) and V.g2_mul_raw(p, R) is not None
    assert V.g2_mul_raw(out["small"], V.SMALL_FACTORS[0]) is None and out["small"] is not None      # of order 10069 (a prime)
    assert V.g2_mul_raw(out["a"], V.COFACTOR * R) is None                     # the twist's group order
    # the reduced multiplication of _pairing.py cannot tell: r mod r = 0
    assert bp.g2_mul(out["a"], R) is None
    # the subgroup's own points: r·Q = O, by the unreduced walk whose last addition is (r − 1)Q + Q
    assert V.g2_mul_raw(bp.G2, R) is None and V.g2_mul_raw(bp.G2, R - 1) == (bp.G2[0], tuple(-c % Q for c in bp.G2[1]))
    assert V.point_flags(2, bp.G2) == 0 and V.point_flags(2, V.G2_ZERO) == V.IDENTITY and V.point_flags(1, bp.G1) == 0


def test_a_good_string_is_accepted(good, rho):
    assert V.judge(good, rho) == (0, (0, 0))
    assert V.judge(good, [0] * len(rho)) == (0, (0, 0))                       # (zero scalars prove nothing — and refuse nothing)


def changed(string, name, index, point):
    a = list(string[name])
    a[index] = point
    return dict(string, **{name: a})


def test_one_thing_wrong_is_that_bit(good, rho):
    n = len(good["tau_g2"])
    s = W.string_scalars(TAU, ALPHA, BETA, POWER)
    # a valid point that is not the next power: the array's ratio alone
    assert V.judge(changed(good, "tau_g1", 5, V.mul(1, s["tau_g1"][5] + 1)), rho) == (V.RATIO_TAU_G1, (0, 0))
    assert V.judge(changed(good, "alpha_g1", n - 1, V.mul(1, s["alpha_g1"][n - 1] + 1)), rho) == (V.RATIO_ALPHA_G1, (0, 0))
    # per-point findings name their place, and no equation is evaluated after them
    g = good["tau_g1"][3]
    assert V.judge(changed(good, "tau_g1", 3, (g[0], (g[1] + 1) % Q)), rho) == (V.OFF_CURVE, (1, 3))
    assert V.judge(changed(good, "beta_g1", 2, V.G1_ZERO), rho) == (V.IDENTITY, (4, 2))
    assert V.judge(changed(good, "tau_g2", 2, V.outside_points()["mixed"]), rho) == (V.SUBGROUP, (2, 2))
    assert V.judge(changed(good, "tau_g1", 0, V.mul(1, 2)), rho) == (V.FIRST, (1, 0))
    assert V.judge(changed(good, "beta_g2", 0, V.mul(2, BETA + 1)), rho) == (V.BETA, (0, 0))


def test_the_chunks_add_up_to_the_combination():
    s = V.base_scalars()
    assert len(s) == V.BASE_N and (s[V.RLC_CHUNK] + 2 * s[0]) % R == 0
    for group in (1, 2):
        cases = V.rlc_cases(group)
        assert {int(name.split("/")[0]) for name in cases} == set(V.RLC_PAIRS[group])
        for name, rho in cases.items():
            want = V.rlc_scalars(s, rho)
            for shift in (0, 1):
                chunks = V.rlc_chunk_scalars(s, rho, shift)
                assert len(chunks) == -(-len(rho) // V.RLC_CHUNK) and sum(chunks) % R == want[shift], name
            if name.endswith("/zero"):
                assert want == (0, 0)
            if name.endswith("/opposite"):
                c = V.rlc_chunk_scalars(s, rho, 0)
                assert c[0] and (c[0] + c[1]) % R == 0 and (len(c) == 2 or c[-1])
            if name.endswith("/equal"):
                c = V.rlc_chunk_scalars(s, rho, 0)
                assert c[0] == 0 and c[1] and c[1] == c[2]


def test_every_kind_of_bad_point_stands_at_every_place():
    for group in (1, 2):
        kinds = V.bad_points(group)
        for kind, (p, flag) in kinds.items():
            assert V.point_flags(group, p) == flag, kind
        seen = set()
        for name, (s, bad) in V.flags_cases(group).items():
            n = len(s)
            assert sorted(bad) == [0, n // 2, n - 1] and 0 not in s
            seen |= {(n, j, kind) for j, kind in enumerate(bad[p] for p in sorted(bad))}
        assert seen == {(n, j, kind) for n in V.FLAGS_N for j in range(3) for kind in kinds}
