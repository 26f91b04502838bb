"""k_cf_open_chains (vimz_amd/csrc/decider_chains.hip): the commitment-opening chains of the full decider's check 5 on the GPU, against plain Python integers
(tests/_cf_chains_ref.py, checked on the CPU by tests/test_cf_chains_ref_host.py) through the launcher the prover calls, and end to end — the decider's
assignment with the chains from the device equals the one with the chains from the host, word for word, and proves.  Every comparison is exact equality.

Launches of 1, 63, 64, 65 and 257 chains (a wave's edge, a workgroup's edge, past them; every launch fills both openings of the grid), scalars 0, 1,
2^254 − 1 mod q, q − 1, digits 0 1 2 3 in turn, bit 253 alone, bit 252 alone, seeded random ones, one scalar in every chain and different ones; additions
of two points with the same x (G_0 = ±H under scalar 0) must raise the flag."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _cf_chains_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = tmp_path_factory.mktemp("decider_chains")
    r = subprocess.run([sys.executable, "-m", "tests._decider_chains_gpu", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=900,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out / "e2e.json") as fp:
        res = json.load(fp)
    res["arrays"] = np.load(out / "chains.npz")
    return res


def same(got, want, what):
    want = R._words(want)
    if not np.array_equal(got, want):
        assert got.shape == want.shape, f"{what}: {got.size // 4} elements, expected {want.size // 4}"
        k = int(np.flatnonzero((got != want).reshape(-1, 4).any(axis=1))[0])
        raise AssertionError(f"{what}: element {k} of {want.size // 4} is {R._ints(got[4 * k:4 * k + 4])[0]}, expected {R._ints(want[4 * k:4 * k + 4])[0]}")


def test_sizes_cover_the_edges():
    assert {n for n, _ in R.cases().values()} == set(R.SIZES)


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_device_chains_equal_the_reference(probe, name):
    H = tuple(int(c) for c in probe["chains"]["H"])
    assert R.on_curve(H)
    m = probe["chains"][name]
    assert m["bad"] == 0 and tuple(int(c) for c in m["H"]) == H
    want_w, want_e = R.expected(name, H)
    same(probe["arrays"][name + "/ends"], want_e, f"end points of {name}")
    same(probe["arrays"][name + "/wires"], want_w, f"wires of {name}")


@pytest.mark.parametrize("name", R.DEGENERATE)
def test_an_addition_of_points_with_the_same_x_raises_the_flag(probe, name):
    assert probe["chains"][name]["bad"] == 1
    assert probe["chains"]["G0_is_G"]["bad"] == 0      # the same scalars over an honest G_0, launched after them


def test_witness_with_device_chains_equals_the_host_s(probe):
    e = probe["e2e"]
    assert e["witness_wires"] > 2_750_000 and e["witness_nonzero"] > e["witness_wires"] // 4
    assert e["witness_first_difference"] is None, f"wire {e['witness_first_difference']} differs"


def test_decider_proves_with_device_chains(probe):
    e = probe["e2e"]
    assert e["gpu_verify"] == 0 and e["host_verify"] == 0 and e["public_inputs_equal"] is True
    assert e["seconds_gpu"]["chains_gpu"] > 0 and e["seconds_host"]["chains_gpu"] == 0
    assert e["bad_switch"] == e["err_invalid"]


def test_tampered_cyclefold_witness_gets_no_proof_on_the_device_path(probe):
    e = probe["e2e"]
    assert e["poked"] == e["err_unsat"]
    assert e["restored_verify"] == 0 and e["restored_public_inputs_equal"] is True


def test_concurrent_proves_on_one_decider_take_turns(probe):
    """Two vimz_decider_prove calls and one vimz_testing_decider_witness at once on the same full decider, chains on the device: all finish, both proofs
    verify, the assignment is the host's.  (The chains' buffers have a lock of their own beside the context's.)"""
    c = probe["e2e"]["concurrent"]
    for n in ("prove_a", "prove_b"):
        assert c[n] == {"verify": 0, "public_inputs_equal": True}, (n, c[n])
    assert c["witness_equal"] is True, c["witness_equal"]


def test_light_decider_runs_no_chains(probe):
    e = probe["e2e"]
    assert e["light_verify"] == 0 and e["seconds_light"]["chains_gpu"] == 0
