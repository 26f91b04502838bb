"""The element-wise kernels of a fold step — k_fold_cross, k_fold5, k_fresh_cross_neg — and the counting kernels that guard imported proofs, stage by stage
against Python integers (tests/_fold_ref.py, itself checked without a GPU by tests/test_fold_ref_host.py), through hooks of libvimz_hip_testing.so only."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fold_kernels_behind_the_test_hooks():
    """vimz_test_fold_cross, vimz_test_fold5, vimz_test_fresh_cross_neg and vimz_test_count on the layouts the wave ballots of mul_fresh branch on (cycling
    classes, waves that never multiply, one generic lane a wave), at sizes around a wave and with a forced grid that reaches the grid stride, with every option
    of k_fold_cross (fold_E, the lookahead's hasB / r_prev / negB, out absent, separate and aliased with Tin, the boolean-row vector at every nb); then the
    lookahead schedule of launch_fold_and_cross driven through the hooks against the direct fold.  Exact: words in Montgomery form.  The body
    (tests/_fold_hooks_gpu.py) runs in a process of its own on the testing library and reports how many cases of each group it ran."""
    env = dict(os.environ, VIMZ_HIP_LIBRARY="testing")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fold_hooks_gpu.py")], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from tests import _fold_hooks_gpu as body
    want = (f"fold hooks ok: refused {body.N_REFUSED} fold_cross {body.N_FOLD_CROSS} fold5 {body.N_FOLD5} fresh_cross_neg {body.N_FRESH_NEG} count {body.N_COUNT} "
            f"schedule {body.N_SCHEDULE}")
    assert r.stdout.strip().splitlines()[-1] == want, r.stdout[-2000:]
