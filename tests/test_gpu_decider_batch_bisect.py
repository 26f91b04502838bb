"""The bisection of a refused chunk in vimz_decider_verify_batch_ex on the GPU (DeviceStages of vimz_amd/csrc/decider_batch.hip: the subset sums are g16_column_sums
over the rows k_g1_lincomb left on the device): the matrix of tests/test_decider_batch_bisect_host.py with a context.  Words and counts equal the host path's and
the planner model's.  The GPU half is tests/_batch_bisect_gpu.py, one process."""
import json
import os
import subprocess
import sys

import pytest

from tests import _batch_bisect_gpu as G
from tests import _novadecider as nd
from vimz_amd.hip import decider_verify_key, verifying_key_words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_part(tmp_path_factory, part, timeout):
    out = tmp_path_factory.mktemp("batch_bisect_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._batch_bisect_gpu", part, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    return run_part(tmp_path_factory, "decider", 600)["decider"]


@pytest.fixture(scope="module")
def host():
    return G.decider_matrix(None)


@pytest.fixture(scope="module")
def want():
    kw = verifying_key_words(nd.verifier_keys()["contrast"])
    good, wrong = G.decider_items()
    w = {"good": decider_verify_key(kw, *good), 0: decider_verify_key(kw, *wrong[0]), 1: decider_verify_key(kw, *wrong[1])}
    return lambda n, bad: [w[i % 2] if i in bad else w["good"] for i in range(n)]


@pytest.mark.parametrize("name", sorted(G.patterns(7)))
def test_device_words_and_counts_are_the_host_s_and_the_model_s(device, host, want, name):
    bad = G.patterns(7)[name]
    for chunk in G.CHUNKS:
        for leaf in G.LEAVES + ("off",):
            key = f"{name}/{chunk}/{leaf}"
            print(key, device[key])
            assert device[key]["words"] == want(7, bad) == host[key]["words"], key
            assert device[key]["stats"] == G.decider_expected(key) == host[key]["stats"], key
            assert device[key]["fallback_s"] > 0, key


def test_nine_proofs_and_the_default_leaf(device, host, want):
    assert device["nine"]["words"] == want(9, (1, 8)) and device["nine"]["stats"] == [2, 3, 2, 3] == host["nine"]["stats"]
    assert device["nine/off"]["words"] == want(9, (1, 8)) and device["nine/off"]["stats"] == [2, 0, 5, 0]
    assert device["default_leaf"]["words"] == want(7, (6,)) and device["default_leaf"]["stats"] == host["default_leaf"]["stats"]
