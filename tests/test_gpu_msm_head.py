"""The head stages of the MSM on their own (vimz_amd/csrc/msm.hpp): the digit producers (load_scalar, for_each_digit, signed_digit<7>) through both counting sorts
(k_hist_lds / k_prefix_scan / k_scatter_lds, and k_hist / k_scan / k_scatter with agg_atomic_inc), k_accum on crafted sort layouts, the unit sums (k_ones_partial,
k_ones_dense, k_ones_dense_rows), the fused paths (k_msm_small with either tail, k_msm_fixed) and the table builders — through the stage hooks of the testing library,
each launch by the function the product calls.  What a whole MSM cannot tell apart is told apart here: an equivalent recoding (the digits are held against the integer
model entry by entry), a slot of `sorted` written twice or never, every sub-bucket length 4..8 of k_msm_small, its chunk merge at every Q mod 3, k_msm_fixed's padded
tree, k_accum's search over runs of empty buckets and its mid-chain doubling and cancellation, the unit queue filled to exactly 64 and past it.  Every comparison is
exact (counters and entries word for word, points as integers mod p inside the bounds of ec.hpp; no tolerance).  Cases and integer reference: tests/_msm_head_ref.py
(checked on the CPU by tests/test_msm_head_ref_host.py); one child process per group (tests/_msm_head_gpu.py) with VIMZ_HIP_LIBRARY=testing."""
import json
import os
import subprocess
import sys

import pytest

from tests import _msm_head_ref as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group", H.GROUPS)
def test_every_case_of_the_group_is_exact(group, tmp_path):
    out = tmp_path / "result.json"
    r = subprocess.run([sys.executable, "-m", "tests._msm_head_gpu", group, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as fp:
        res = json.load(fp)
    print(r.stdout[-300:])
    cases = H.group_cases(group)
    assert len(cases) > 0
    assert f"msm head {group} cases run: {len(cases)} " in r.stdout, r.stdout[-500:]      # the driver's own count: a group that ran nothing, or less, fails
    assert res["ran"] == len(cases)
    assert res["failed"] == [], f"{len(res['failed'])} of {len(cases)} cases: " + "\n".join(f"{c}: {m}" for c, m in res["failed"][:5])
