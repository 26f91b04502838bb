"""The transform over points of a Groth16 set-up from a powers-of-tau string (vimz_amd/csrc/g16_powers.hip: g16_point_transform — k_pt_twiddles, k_pt_bitrev, one
k_pt_stage per stage, k_scale_points — in G1 and in G2) against plain Python integers, and the calls built on it: vimz_powers_lagrange, hip.lagrange_from_powers.

One probe process per group (tests/_point_transform_gpu.py g1 | g2 | api), so that one group's failure leaves the others' verdicts standing.  Inputs are [s_k]G
made by vimz_test_g16_fixed_mul (pinned on Python integers by tests/test_gpu_g16_kernels.py), the expected outputs [x_j]G made the same way from the scalars
tests/_g16_powers_ref.py derives; SPOT entries of every case are compared with tests._pairing / _g16_ref.g2_gen_mul directly as well.  Every comparison is exact
equality of words.  The sizes put n/2 butterflies at half a block, one block and two blocks of k_pt_stage; the cases hold unit vectors, a constant, identities
(all, and a quarter of the places), and P_k = P_(k + n/2), whose last stage doubles and cancels."""
import json
import os
import random
import subprocess
import sys

import pytest

from tests import _g16_powers_ref as W
from tests import _g16_ref as G
from tests import _point_transform_gpu as P
from tests._g16_kernels_gpu import hex_ints, ints_hex
from tests._pairing import G1, Q, R, g1_mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = 8                         # entries of a case compared with g1_mul / g2_gen_mul
CASES = {group: [(logn, name) for logn in W.TRANSFORM_LOGN[group] for name in W.transform_cases(logn)] for group in (1, 2)}


def run_probe(tmp_path_factory, what):
    out = tmp_path_factory.mktemp("point_transform_" + what) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._point_transform_gpu", what, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def probe_g1(tmp_path_factory):
    return run_probe(tmp_path_factory, "g1")


@pytest.fixture(scope="module")
def probe_g2(tmp_path_factory):
    return run_probe(tmp_path_factory, "g2")


@pytest.fixture(scope="module")
def probe_api(tmp_path_factory):
    return run_probe(tmp_path_factory, "api")


def point_words(group, s):
    """[s]G as the hooks write it"""
    if group == 1:
        p = g1_mul(G1, s)
        return [0, 0] if p is None else [p[0], p[1]]
    return G.g2_words(G.g2_gen_mul(s))


def check_case(probe, group, logn, name):
    n, per = 1 << logn, 2 * group                         # per: coordinates of a point
    s = W.transform_cases(logn)[name]
    want = W.transform_expected(s, logn, name)
    run = probe["runs"][f"{logn}/{name}"]
    assert set(run["out"]) == set(want) == ({"fwd", "inv", "inv_scaled", "back_unscaled", "back"} if name in W.FULL_CASES else {"fwd"})
    width = 64 * per
    for what in want:
        got, exp = run["out"][what], run["want"][what]
        assert len(got) == len(exp) == width * n
        assert got == exp, f"G{group} logn {logn} {name} {what}: element {next(j for j in range(n) if got[width * j:width * j + width] != exp[width * j:width * j + width])} differs"
    # the expected points themselves, and the inputs, on Python integers
    pin, pout = hex_ints(run["in"]), hex_ints(run["out"]["fwd"])
    spot = range(n) if n <= SPOT else sorted({0, 1, n // 2, n - 1} | set(random.Random(f"g16/transform/spot/{group}/{logn}/{name}").sample(range(n), SPOT - 4)))
    for j in spot:
        assert pin[per * j:per * j + per] == point_words(group, s[j]), f"input {j}"
        assert pout[per * j:per * j + per] == point_words(group, want["fwd"][j]), f"output {j}"
    assert all(c < Q for c in pout)
    if name in W.FULL_CASES:
        assert run["out"]["back"] == run["in"]                                          # forward, then the scaled inverse: the input itself
        assert want["back_unscaled"] == [n * x % R for x in s]
    if name == "e_0":
        assert pout == point_words(group, 1) * n                                        # n copies of the generator
    if name == "identity":
        assert not any(pout)


@pytest.mark.parametrize("logn,name", CASES[1])
def test_transform_g1(probe_g1, logn, name):
    check_case(probe_g1, 1, logn, name)


@pytest.mark.parametrize("logn,name", CASES[2])
def test_transform_g2(probe_g2, logn, name):
    check_case(probe_g2, 2, logn, name)


def test_the_cases_hold_what_they_are_meant_to():
    assert W.TRANSFORM_LOGN == {1: (1, 2, 3, 6, 7, 8), 2: (1, 2, 3, 7)}
    assert {(1 << logn) // 2 for logn in (6, 7, 8)} == {W.PT_BLOCK // 2, W.PT_BLOCK, 2 * W.PT_BLOCK}
    assert set(W.transform_cases(3)) == {"random", "e_0", "e_1", "constant", "identity", "holes", "half_period"}


# ---- vimz_powers_lagrange, hip.lagrange_from_powers -------------------------------------------------------------------------------------------------
def mont_hex(canonical_hex):
    """the words of the same coordinates in the `.ptau` file's Montgomery form"""
    return ints_hex([c * (1 << 256) % Q for c in hex_ints(canonical_hex)])


@pytest.mark.parametrize("logn", P.API_LOGN)
def test_lagrange_bases_of_a_known_string(probe_api, logn):
    n = 1 << logn
    sc = W.string_scalars(P.API_TAU, P.API_ALPHA, P.API_BETA, P.API_POWER)
    closed = W.lagrange_closed_form(P.API_TAU, logn)
    got = probe_api["bases"][str(logn)]
    assert set(got["mont"]) == {"tau_g1", "alpha_g1", "beta_g1", "tau_g2"}
    for (name, group), factor in zip(P.API_ARRAYS, (1, P.API_ALPHA, P.API_BETA, 1)):
        assert got["shape"][name] == [n, 8 * group]
        assert got["want"][name] == got["want_closed"][name]                            # the transform of the string's scalars is the closed form of L_j(tau)
        assert W.lagrange(sc[name], logn) == [factor * x % R for x in closed]
        assert got["canonical"][name] == got["want"][name], name                        # the ABI on canonical words
        assert got["mont"][name] == mont_hex(got["want"][name]), name                   # lagrange_from_powers on the file's form
        words = hex_ints(got["canonical"][name])
        for j in (0, n - 1):
            assert words[2 * group * j:2 * group * (j + 1)] == point_words(group, factor * closed[j] % R), (name, j)
    assert hex_ints(probe_api["string"]["tau_g1"])[2:4] == point_words(1, P.API_TAU)


@pytest.mark.parametrize("logn", P.API_LOGN)
def test_commitment_by_evaluations_equals_commitment_by_coefficients(probe_api, logn):
    c = probe_api["commit"][str(logn)]
    assert c["by_evaluations"] == c["by_coefficients"]
    coef = G.interpolate(P.API_EVALS[:1 << logn], logn)
    assert hex_ints(c["by_evaluations"]) == point_words(1, G.horner(coef, P.API_TAU))


def test_command_line_form_writes_the_same_bases(probe_api):
    cli = probe_api["cli"]
    assert cli["rc"] == 0 and cli["logn"] == P.API_POWER and cli["usage_rc"] == 2
    assert cli["arrays"] == probe_api["bases"][str(P.API_POWER)]["mont"]


def test_refusals_and_a_good_call_after_them(probe_api):
    assert set(probe_api["refused"]) == {"null_ctx", "null_points", "null_out", "group_0", "group_3", "logn_0", "logn_27", "short_g1", "short_g2", "g1_not_reduced",
                                         "g2_not_reduced", "g1_off_curve", "g2_off_curve", "mont_not_reduced"}
    assert all(rc == probe_api["invalid"] for rc in probe_api["refused"].values()), probe_api["refused"]
    acc, want = probe_api["accepted"], probe_api["bases"][str(P.API_POWER)]["want"]
    assert acc["g1"] == 0 and acc["g2"] == 0
    assert acc["g1_out"] == want["tau_g1"] and acc["g2_out"] == want["tau_g2"]
