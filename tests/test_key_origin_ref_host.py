"""The reference of vimz_decider_key_verify_origin (tests/_key_origin_ref.py) on the CPU: its verdict on scalars accepts the keys _g16_powers_ref.derive_key derives for
random small circuits — domains 2 to 128, unit rows filling the last slot and not, one private wire and many, wires no matrix touches — and those keys after a
contribution; every tamper is refused with bits that name what was tampered with; and on the smallest shape the same verdict on key BYTES over tests/_pairing.py's
points and pairings agrees with it, before and after _key_contrib_ref.contribute."""
import pytest

from tests import _key_contrib_ref as K
from tests import _key_origin_ref as O
from tests._pairing import R

SHAPES = O.DRIVER_SHAPES + (O.TAMPER_SHAPE, (2, 1, 1, "full"), (4, 0, 5, "half"))


@pytest.mark.parametrize("shape", SHAPES)
def test_derived_and_contributed_keys_are_accepted(shape):
    circ = O.circuit(*shape)
    string = O.string_of(circ["logn"])
    rho, rho_h = O.fixed_rho(circ)
    key = O.derived_key(circ, string)
    bits, first, points = O.verdict(key, circ, string, rho, rho_h)
    assert (bits, first) == (0, (0, 0)), O.bit_names(bits)
    assert points[0] == points[6] and points[1] == points[7] and points[2] == points[8] and points[3] == points[9]
    assert points[4] * key["delta2"] % R == points[10] and points[5] * key["delta2"] % R == points[11]
    assert O.verdict(O.contributed(key, K.DELTAS[0]), circ, string, rho, rho_h)[:2] == (0, (0, 0))
    # a longer string serves a shorter domain
    assert O.verdict(key, circ, O.string_of(circ["logn"] + 1), rho, rho_h)[:2] == (0, (0, 0))


def test_the_shapes_cover_what_the_issue_names():
    shapes = [O.circuit(*s) for s in O.DRIVER_SHAPES]
    assert {c["logn"] for c in shapes} == {1, 3, 6, 7} and {c["n_pub"] for c in shapes} == {0, 2, 13}
    assert any(c["m"] - c["n_pub"] - 1 == 1 for c in shapes) and any(c["m"] - c["n_pub"] - 1 > 20 for c in shapes)
    assert any(c["n_c"] + c["n_pub"] + 1 == c["n"] for c in shapes) and any(c["n_c"] + c["n_pub"] + 1 < c["n"] for c in shapes)
    big = O.circuit(*O.DRIVER_SHAPES[3])
    key = O.derived_key(big, O.string_of(big["logn"]))
    assert key["a"][-1] == key["a"][-2] == key["b1"][-1] == key["l"][-1] == 0                  # wires nobody touches
    assert sum(1 for s in key["b2"] if s == 0) > big["m"] // 2                                # most of b2 is the identity


def test_every_tamper_is_refused_with_the_bits_of_what_it_touched():
    circ = O.circuit(*O.TAMPER_SHAPE)
    string = O.string_of(circ["logn"])
    rho, rho_h = O.fixed_rho(circ)
    table = O.tampers(circ, string)
    assert set(O.REQUIRED_TAMPERS) <= set(table)
    got = {name: O.verdict(t["key"], t["circuit"], t["string"], rho, rho_h)[:2] for name, t in table.items()}
    assert all(bits for bits, _f in got.values()), got
    want = {"a_point_replaced": (O.A, (0, 0)), "b1_point_replaced": (O.B1, (0, 0)), "b2_point_replaced": (O.B2, (0, 0)), "ic_point_replaced": (O.IC, (0, 0)),
            "l_point_replaced": (O.L, (0, 0)), "h_point_replaced": (O.H, (0, 0)), "a_compensating_pair": (O.A, (0, 0)), "l_scaled_by_another_delta": (O.L, (0, 0)),
            "h_of_half_the_domain": (O.H, (0, 0)), "kzg_swapped": (O.FIXED_POINTS, (O.AT_FIXED, 0)), "alpha1_swapped": (O.FIXED_POINTS, (O.AT_FIXED, 1)),
            "beta1_swapped": (O.FIXED_POINTS, (O.AT_FIXED, 2)), "beta2_swapped": (O.FIXED_POINTS, (O.AT_FIXED, 3)), "gamma2_swapped": (O.FIXED_POINTS, (O.AT_FIXED, 4)),
            "delta1_changed": (O.DELTA, (0, 0)), "key_of_another_tau": (O.FIXED_POINTS, (O.AT_FIXED, 0)), "header_m_off_by_one": (O.HEADER, (O.AT_HEADER, 1)),
            "l_point_off_curve": (O.OFF_CURVE, (O.AT_L, 0)), "a_coordinate_is_q": (O.COORD, (O.AT_A, circ["m"] - 1))}
    for name, w in want.items():
        assert got[name] == w, (name, O.bit_names(got[name][0]), got[name][1])
    assert got["b2_point_off_the_subgroup"][0] == O.SUBGROUP and got["b2_point_off_the_subgroup"][1][0] == O.AT_B2
    # a coefficient of A shows in the a query and in whichever of ic and l holds its wire; of B in b1, b2 and one of them; of C in one of them alone
    for X, own in (("A", O.A), ("B", O.B1 | O.B2), ("C", 0)):
        bits = got[f"circuit_{X}_coefficient"][0]
        assert bits & (O.A | O.B1 | O.B2) == own and bits & (O.IC | O.L) and not bits & ~(own | O.IC | O.L), (X, O.bit_names(bits))


def test_the_key_of_another_tau_fails_every_equation_once_its_kzg_point_is_put_right():
    circ = O.circuit(*O.TAMPER_SHAPE)
    string = O.string_of(circ["logn"])
    rho, rho_h = O.fixed_rho(circ)
    key = dict(O.tampers(circ, string)["key_of_another_tau"]["key"], kzg=string["tau_g2"][1])
    assert O.verdict(key, circ, string, rho, rho_h)[0] == O.A | O.B1 | O.B2 | O.IC | O.L | O.H


def test_the_h_scalars_are_the_combination_of_the_differences():
    n, rng = 8, __import__("random").Random(5)
    rho_h, t = [rng.getrandbits(128) for _ in range(n - 1)], [rng.randrange(R) for _ in range(2 * n - 1)]
    s = O.h_scalars(rho_h, n)
    assert s[n - 1] == 0 and sum(x * y for x, y in zip(s, t)) % R == sum(r * (t[j + n] - t[j]) for j, r in enumerate(rho_h)) % R


@pytest.fixture(scope="module")
def smallest():
    circ = O.circuit(1, 0, 1, "full")
    string = O.string_of(circ["logn"])
    return circ, string, O.string_points_of(string), O.fixed_rho(circ)


def test_the_verdict_on_bytes_agrees_for_a_derived_and_a_contributed_key(smallest):
    circ, string, pts, (rho, rho_h) = smallest
    key = O.derived_key(circ, string)
    blob = O.blob_of(key)
    assert K.layout(blob)["m"] == circ["m"]
    assert O.verify_points(blob, circ, pts, rho, rho_h) == (0, (0, 0))
    after, _rec = K.contribute(blob, K.DELTAS[0], K.NONCES[0])
    assert after == O.blob_of(O.contributed(key, K.DELTAS[0]))
    assert O.verify_points(after, circ, pts, rho, rho_h) == (0, (0, 0))


@pytest.mark.parametrize("name", ("l_point_replaced", "delta1_changed", "gamma2_swapped", "l_point_off_curve", "circuit_A_coefficient"))
def test_the_verdict_on_bytes_agrees_for_a_tampered_key(smallest, name):
    circ, string, pts, (rho, rho_h) = smallest
    t = O.tampers(circ, string)[name]
    blob = O.apply_patch(O.blob_of(O.derived_key(circ, string)), t)
    assert O.verify_points(blob, t["circuit"], pts, rho, rho_h) == O.verdict(t["key"], t["circuit"], t["string"], rho, rho_h)[:2]
