"""Judging on the GPU that a decider key derives from a powers-of-tau string and the circuit (vimz_decider_key_verify_origin; vimz_amd/csrc/g16_key_origin.hip): the new
kernel through its hook, the driver on synthetic circuits, and once the product call on the light decider of the hash step.

k_spmv3_dict (one launch over a grid of (rows, 3), a thread a row) runs over tests/_key_origin_ref.spmv_cases() and is compared WORD FOR WORD with Python integers: n_c = 1,
63, 64, 65, 257; a tail of one row, of many, and none (n_c = n); rows empty and of 1, 64, 65 and 700 terms; a first, a last and every row empty; the column m − 1; a row
that names a column twice; coefficients 0, 1, r − 1 and full width; v holding 0, 2^128 − 1 and r − 1; three matrices of different shapes in each call.  (One path: there is
no short/long threshold to stand around.)
The driver (vimz_test_key_origin: the product's function on a caller's R1CS with a given rho) runs over logn = 1, 3, 6, 7, n_pub = 0, 2, 13, one private wire and many,
wires no matrix touches: its eleven intermediate points equal [s]G of the reference's scalars (made by vimz_test_g16_fixed_mul, pinned on Python integers by
tests/test_gpu_g16_kernels.py) word for word, the derived key and the key after one contribution are accepted, and every tamper yields exactly the bits and first_bad
tests/_key_origin_ref.verdict derives (a missed equation has probability at most 2^-128).  The GPU half is tests/_key_origin_gpu.py, a process per part."""
import json
import os
import subprocess
import sys

import pytest

from tests import _key_origin_ref as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["/".join(str(x) for x in s) for s in O.DRIVER_SHAPES]


def run_part(tmp_path_factory, part, timeout):
    out = tmp_path_factory.mktemp("key_origin_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._key_origin_gpu", part, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return run_part(tmp_path_factory, "kernels", 600)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return run_part(tmp_path_factory, "driver", 600)


@pytest.fixture(scope="module")
def decider(tmp_path_factory):
    return run_part(tmp_path_factory, "decider", 900)


@pytest.mark.parametrize("name", sorted(O.spmv_cases()))
def test_the_three_products_word_for_word(kernels, name):
    from tests._g16_kernels_gpu import hex_ints
    got = kernels["spmv"][name]
    assert got["rc"] == 0
    assert [hex_ints(h) for h in got["out"]] == O.spmv_expected(O.spmv_cases()[name]), name


def test_a_matrix_with_an_index_out_of_bounds_is_refused_before_any_launch(kernels):
    assert set(kernels["refused"]) == {"column_is_m", "coefficient_index", "offsets_decrease", "offsets_overrun"}
    for name, (rc, message) in kernels["refused"].items():
        assert rc == kernels["invalid"] and message.startswith("vimz_test_g16_spmv_dict: matrix A:"), (name, message)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_driver_accepts_a_derived_key_and_its_points_are_the_references(driver, shape):
    got = driver["shapes"][shape]
    assert (got["rc"], got["result"], got["first_bad"]) == (0, 0, [0, 0]), (O.bit_names(got["result"]), got["message"])
    assert got["points"] == got["want_points"]                         # key side a, b1, b2, ic, l, h; string side a, b1, b2, K(P), K(Q), h
    words = bytes.fromhex(got["points"])
    assert words[:64 * 5] == words[64 * 7:64 * 12] and any(words[:64])     # a, b1, b2, ic: the two sides are the same points, and not the identity


@pytest.mark.parametrize("shape", SHAPES)
def test_the_driver_accepts_the_key_after_a_contribution(driver, shape):
    got = driver["shapes"][shape]
    assert got["contributed_is_the_reference"]
    c = got["contributed"]
    assert (c["rc"], c["result"], c["first_bad"]) == (0, 0, [0, 0]), O.bit_names(c["result"])
    a, b = bytes.fromhex(c["points"]), bytes.fromhex(got["points"])
    assert a[:64 * 5] == b[:64 * 5] and a[64 * 5:64 * 6] != b[64 * 5:64 * 6] and a[64 * 6:64 * 7] != b[64 * 6:64 * 7] and a[64 * 7:] == b[64 * 7:]      # only the sums over l and h moved


@pytest.fixture(scope="module")
def tamper_table():
    circ = O.circuit(*O.TAMPER_SHAPE)
    string = O.string_of(circ["logn"])
    rho, rho_h = O.fixed_rho(circ)
    return {name: O.verdict(t["key"], t["circuit"], t["string"], rho, rho_h)[:2] for name, t in O.tampers(circ, string).items()}


@pytest.mark.parametrize("name", O.REQUIRED_TAMPERS + ("l_point_off_curve", "a_coordinate_is_q"))
def test_a_tampered_key_yields_exactly_the_references_bits(driver, tamper_table, name):
    bits, first = tamper_table[name]
    got = driver["tampers"][name]
    assert bits and got["rc"] == 0                                                 # a verdict, not an error
    assert (got["result"], tuple(got["first_bad"])) == (bits, first), f"{name}: got {O.bit_names(got['result'])} at {got['first_bad']}, the reference {O.bit_names(bits)} at {first}"


def test_every_tamper_of_the_reference_ran(driver, tamper_table):
    assert set(driver["tampers"]) == set(tamper_table) >= set(O.REQUIRED_TAMPERS)


def test_a_longer_string_serves_and_the_refusals_are_errors_with_their_messages(driver):
    got = driver["longer_string"]
    assert (got["rc"], got["result"]) == (0, 0)
    want = {"truncated": "wrong length", "wrong_magic": "not a decider key", "tau_g1_a_point_short": "the string is shorter than the key's domain",
            "powers_a_point_short": "the string is shorter than the key's domain", "string_point_off_curve": "the string: a point is not on its curve"}
    assert set(driver["refused"]) == set(want)
    for name, text in want.items():
        got = driver["refused"][name]
        assert got["rc"] == driver["invalid"] and got["message"].startswith("vimz_decider_key_verify_origin: " + text), (name, got["message"])


# ---- the product call, once: the light decider of the hash step -------------------------------------------------------------------------------------------
def test_the_saved_key_of_a_set_up_from_the_string_is_accepted(decider):
    assert decider["info"]["domain"] == 1 << 18
    assert decider["saved_key"] == [0, [0, 0]] and decider["contributed_key"] == [0, [0, 0]] and decider["good_string_verified"] == [0, [0, 0]]
    assert decider["trapdoor_key_of_the_strings_scalars"] == [0, [0, 0]]
    assert len(decider["seconds"]) == 5 and all(x > 0 for x in decider["seconds"])
    print("vimz_decider_key_verify_origin on the light hash decider's key, seconds {synthesis, host conversion + fixed words, flags, circuit side, combinations + pairings}:", decider["seconds"])


def test_other_keys_are_refused_with_their_bits(decider):
    assert decider["trapdoor_key_of_another_alpha"] == [O.FIXED_POINTS, [O.AT_FIXED, 1]]
    assert decider["poked_l"] == [O.L, [0, 0]] and decider["poked_b2"] == [O.B2, [0, 0]]
    assert decider["b2_identities"] > 0
    assert decider["other_mode"][0] == O.HEADER and decider["other_mode"][1][0] == O.AT_HEADER
    assert len(decider["problems"]) == 2


def test_a_bad_string_is_refused_before_any_key_work(decider):
    code, message = decider["bad_string_verified"]
    assert code == decider["invalid"] and "verify_key_origin: the powers-of-tau string is refused" in message      # (hip.verify_powers' refusal, not the library's: no key work was done)
    code, message = decider["short_string"]
    assert code == decider["invalid"] and "the string is shorter than the key's domain" in message


def test_the_command(decider):
    cli = decider["cli"]
    assert cli["good"]["rc"] == 0 and "accepted" in cli["good"]["stdout"]
    assert cli["bad"]["rc"] == 1 and "REFUSED" in cli["bad"]["stdout"] and " B2)" in cli["bad"]["stdout"]
    assert cli["usage"]["rc"] == 2
