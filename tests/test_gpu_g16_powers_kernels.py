"""The point kernels of a Groth16 set-up from a powers-of-tau string (vimz_amd/csrc/g16_powers.hip) against plain Python integers, through a hook that calls the
very function the set-up is to call.  Built so far, and so tested: the same-scalar multiplication out_i = k·P_i over G1 (g16_scale_points, k_scale_points).

Inputs are [s_i]G1 made by vimz_test_g16_fixed_mul (pinned on Python integers by tests/test_gpu_g16_kernels.py), the expected outputs [k·s_i]G1 made the same
way; SPOT entries of every case are compared with tests._pairing.g1_mul directly as well.  Every comparison is exact equality of words.  Scalars 0, 1, 2, r − 1
and a full-size one; n at the kernel's block of 64 threads − 1, + 0, + 1; the identity at the first and at a middle place of every input."""
import json
import os
import random
import subprocess
import sys

import pytest

from tests import _g16_powers_ref as W
from tests._g16_kernels_gpu import hex_ints
from tests._pairing import G1, Q, R, g1_mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = 8                         # entries of a case compared with g1_mul


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = tmp_path_factory.mktemp("g16_powers") / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._g16_powers_gpu", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


def point_words(p):
    return [0, 0] if p is None else [p[0], p[1]]


SCALARS = {**W.scale_scalars(), "zero": 0}


@pytest.mark.parametrize("name", sorted(SCALARS))
@pytest.mark.parametrize("n", W.SCALE_N)
def test_same_scalar_multiplication(probe, n, name):
    k, s = SCALARS[name], W.scale_points(n)
    got = probe["scale"][f"{n}/{name}"]
    assert got["out"] == got["want"], f"{name}·P over {n} points: element {next(i for i in range(n) if got['out'][128 * i:128 * i + 128] != got['want'][128 * i:128 * i + 128])} differs"
    pin, pout = hex_ints(got["in"]), hex_ints(got["out"])
    assert len(pin) == len(pout) == 2 * n
    spot = sorted({0, 1, n // 2, n - 1} | set(random.Random(f"g16/powers/spot/{n}").sample(range(n), SPOT - 4)))
    for i in spot:
        assert pin[2 * i:2 * i + 2] == point_words(g1_mul(G1, s[i])), f"input {i}"
        assert pout[2 * i:2 * i + 2] == point_words(g1_mul(G1, k * s[i] % R)), f"output {i}"
    for i in range(n):
        x, y = pout[2 * i:2 * i + 2]
        if s[i] == 0 or k == 0:
            assert (x, y) == (0, 0)                                                     # the identity stays the identity; 0·P is the identity
        else:
            assert x < Q and y < Q and (y * y - x * x * x - 3) % Q == 0 and (x, y) != (0, 0)
    if name == "one":
        assert pout == pin
    if name == "minus_one":
        assert pout == [v if j % 2 == 0 or v == 0 else Q - v for j, v in enumerate(pin)]      # −P = (x, q − y)


def test_the_cases_hold_what_they_are_meant_to():
    assert set(W.SCALE_N) == {W.PT_BLOCK - 1, W.PT_BLOCK, W.PT_BLOCK + 1}
    assert {1, 2, R - 1} <= set(SCALARS.values()) and SCALARS["random"].bit_length() >= 251
    assert all(W.scale_points(n)[0] == 0 and W.scale_points(n)[n // 2] == 0 for n in W.SCALE_N)


def test_bad_arguments_are_refused(probe):
    assert set(probe["refused"]) == {"n_0", "scalar_r", "off_curve", "x_not_reduced"}
    assert all(rc == probe["invalid"] for rc in probe["refused"].values()), probe["refused"]
    assert probe["accepted"] == 0
