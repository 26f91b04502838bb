"""hip.kzg_from_powers: KZG's keys taken from a powers-of-tau string instead of a tau drawn in the process.  The string's points [tau^k]G1, [tau^k]G2 for a tau
chosen here are made by vimz_test_g16_fixed_mul (pinned on Python integers by tests/test_gpu_g16_kernels.py), written into a `.ptau` container and read back by
iden3.read_ptau; the srs must then hold the first n of them word for word, vk must be [tau]G2, and a commitment under the srs must be [sum s_k tau^k]G1.  n = 2
(the least the decider's pairing check can use), an odd n and the whole string; the refusals.  SPOT points are compared with tests._pairing directly."""
import json
import os
import subprocess
import sys

import pytest

from tests import _g16_powers_gpu as P
from tests import _g16_ref as G
from tests._g16_kernels_gpu import hex_ints
from tests._pairing import G1, G2, R, g1_mul, g2_mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = (0, 1, 2, 14)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = tmp_path_factory.mktemp("kzg_from_powers") / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._g16_powers_gpu", str(out), "kzg"], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


def test_the_string_is_the_powers_of_tau(probe):
    pts = hex_ints(probe["tau_g1"])
    assert len(pts) == 2 * ((2 << P.KZG_POWER) - 1)
    for k in SPOT:
        assert tuple(pts[2 * k:2 * k + 2]) == g1_mul(G1, pow(P.KZG_TAU, k, R)), k
    assert hex_ints(probe["tau_g2_1"]) == G.g2_words(g2_mul(G2, P.KZG_TAU))


@pytest.mark.parametrize("n", P.KZG_N)
def test_srs_and_vk_are_the_strings_points(probe, n):
    got = probe["srs"][str(n)]
    assert got["n"] == n and got["vk_shape"] == [4, 4]
    assert got["points"] == probe["tau_g1"][:128 * n]                      # the first n powers, canonical, word for word
    assert got["vk"] == probe["tau_g2_1"]                                  # [tau]G2, canonical


@pytest.mark.parametrize("n", P.KZG_N)
def test_a_commitment_under_the_srs(probe, n):
    c = probe["commit"][str(n)]
    assert c["got"] == c["want"]
    sc = (P.KZG_SCALARS * n)[:n]
    assert tuple(hex_ints(c["got"])) == g1_mul(G1, sum(s * pow(P.KZG_TAU, k, R) for k, s in enumerate(sc)) % R)


def test_refusals(probe):
    assert set(probe["refused"]) == {"n_1", "n_above", "not_generator", "vk_not_reduced", "one_g2_power"}
    assert all(rc == probe["invalid"] for rc in probe["refused"].values()), probe["refused"]
