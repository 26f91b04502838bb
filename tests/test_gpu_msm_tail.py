"""The tail stages of the large MSM on their own (vimz_amd/csrc/msm.hpp: k_scan / k_prefix_scan, k_combine with its three kinds of workgroups and the ticketed
two-stage fold, k_reduce, k_reduce_planes, k_tree256, k_tree_rows) and the four-lane additions under them (ec_mem.hpp: quad_level, quad_tree256 — identity, copy and
same-x modes, the wave skip), through the stage hooks of the testing library, each launch by the launcher the product calls.  Raw XYZZ slots go in — any
representative inside the bounds of ec.hpp: lifted coordinates, other z, the same point twice in one quad, Q next to −Q, identities on either side — and the
kernel's own representative comes back; every comparison is exact (integers mod p, the bounds, limbs word for word where the contract fixes them; no tolerance).
What a whole MSM over random scalars never builds is built here: a split-heavy bucket with a short last part, a heavy list past position 1023, one that overflowed,
tickets met a second time.  Cases and integer reference: tests/_msm_tail_ref.py (checked on the CPU by tests/test_msm_tail_ref_host.py); one child process per group
(tests/_msm_tail_gpu.py) with VIMZ_HIP_LIBRARY=testing."""
import json
import os
import subprocess
import sys

import pytest

from tests import _msm_tail_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group", T.GROUPS)
def test_every_case_of_the_group_is_exact(group, tmp_path):
    out = tmp_path / "result.json"
    r = subprocess.run([sys.executable, "-m", "tests._msm_tail_gpu", group, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as fp:
        res = json.load(fp)
    cases = T.group_cases(group)
    assert len(cases) > 0
    assert f"msm tail {group} cases run: {len(cases)} " in r.stdout, r.stdout[-500:]      # the driver's own count: a group that ran nothing, or less, fails
    assert res["ran"] == len(cases)
    assert res["failed"] == [], f"{len(res['failed'])} of {len(cases)} cases: " + "\n".join(f"{c}: {m}" for c, m in res["failed"][:5])
