"""The lazily reduced 9 x 29-bit field (vimz_amd/csrc/fp29.hpp) on the device, one operation at a time on raw operands (vimz_test_fp29_probe, a hook
of libvimz_hip_testing.so only): structured and random in-contract operands of every operation in all four fields against Python integers —
residue, limb normalisation, documented bound — and limb for limb against the host build of the same function (tests/_fp29_ref.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fp29_on_the_device_matches_integers_and_the_host_build(tmp_path):
    import re
    from tests import _fp29_ref as ref
    env = dict(os.environ, VIMZ_HIP_LIBRARY="testing")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fp29_probe_gpu.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"fp29 probe ok: (\d+) blocks, (\d+) cases, at least (\d+) a block", r.stdout)
    assert m, r.stdout[-2000:]
    blocks, cases, least = (int(x) for x in m.groups())
    # every operation in every field, each with its 20 000 random operands on top of at least 300 structured ones (the bar of the host run)
    assert blocks == 4 * len(ref.OPS), f"{blocks} blocks checked on the device, {4 * len(ref.OPS)} expected"
    assert least >= ref.RANDOM_PER_OP + 300 and cases >= blocks * (ref.RANDOM_PER_OP + 300), f"too few cases: {cases} in all, {least} in the smallest block"
