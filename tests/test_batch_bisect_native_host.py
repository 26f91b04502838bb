"""The C++ bisection planner (vimz_amd/csrc/batch_bisect.hpp) on the CPU: tests/native/batch_bisect_check.cpp, built with g++ -fsanitize=address,undefined and run
directly, runs it over every bad subset of c = 1…9 members (leaf 1…4, chunks of c, 4 and 2, one side and two) with a callback that knows the bad set; its traces
must be those of tests/_batch_bisect_ref.py, and the run must end without a sanitizer report.  No GPU."""
import os
import subprocess

import pytest

from tests import _batch_bisect_ref as B
from tests.test_batch_bisect_ref_host import SIDE_PATTERNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = tmp_path_factory.mktemp("batch_bisect") / "batch_bisect_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "batch_bisect_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-4000:]
    return out.stdout.splitlines()


def _subsets(text):
    return [(int(t.split("-")[0]), int(t.split("-")[1].split(":")[0]), int(t.split(":")[1])) for t in text.split()]


def test_the_planner_s_traces_are_the_model_s(native):
    assert native[-1] == f"done cases={len(native) - 1}" and len(native) - 1 == sum(1 << c for c in range(1, 10)) * 4 * 3 * 3
    worst = {}
    for line in native[:-1]:
        head, asked, singles, counts = line.split("|")
        c, leaf, chunk, pattern, badset = (int(t) for t in head.split())
        bad = {i: SIDE_PATTERNS[pattern](i) for i in range(c) if (badset >> i) & 1}
        roots = B.chunks_of(c, chunk or c)
        want = B.plan(roots, bad, leaf)
        assert _subsets(asked) == want["asked"] and _subsets(singles) == want["singles"], line
        assert [int(t) for t in counts.split()] == want["stats"] + [want["subsets"]], line
        # the bound, as a condition on the planner itself: at most 2·(members − 1) subsets asked over the refused chunks
        bound = sum(2 * (hi - lo - 1) for lo, hi in roots if any(i in bad for i in range(lo, hi)))
        assert want["subsets"] <= bound, line
        worst[c] = max(worst.get(c, 0), want["subsets"])
    assert worst == {c: 2 * (c - 1) for c in range(1, 10)}
