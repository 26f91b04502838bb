"""The MSM's host-side decisions (vimz_amd/csrc/msm_shape.hpp: path, window plan, every size the launchers reserve and launch from) compiled
with g++ and compared with values derived by hand from the launcher the function replaced — no GPU, no HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LARGE_30721 = dict(path="LARGE", c=9, K=29, nbw=256, nb=7424, lds_sort=1, sub=8, entries=890909, max_subs=118788, sort_blocks=32, lane_bits=1, heavy_min=32,
                   kout=29, tabled=0)
SHARED_305185 = dict(path="LARGE", tabled=1, c=15, K=17, nbw=16384, nb=16384, lds_sort=1, sub=16, entries=5188145, max_subs=340644, sort_blocks=74, lane_bits=1,
                     heavy_min=32, bstride=0, pstride=313321, vw=1024, V=16, kout=32, sums=32)

# case id -> "invalid" / "not-supported" / the fields that must hold (254-bit scalars unless the case says otherwise)
EXPECTED = {
    "1": dict(path="SMALL", c=7, K=37, nbw=64, nb=2368, tabled=0, Q=1, chunk=1536),
    "2": dict(path="SMALL", Q=2, chunk=769),
    "3": dict(path="SMALL", Q=20, chunk=1536, sums=37),
    "4": LARGE_30721,
    "5": LARGE_30721,                                       # VIMZ_DEBUG_NO_SMALL_MSM changes nothing above the fused path's limit
    "6": dict(path="LARGE", c=7, K=37),                     # ... and below it the window is msm_plan's
    "7": SHARED_305185,
    "8": dict(SHARED_305185, sub=8, max_subs=664903, sums=33, split_ones=1),
    "9": dict(path="LARGE", tabled=4, planes=1, Pl=14, Gp=16, kout=16),
    "9g": "not-supported",
    "10": dict(SHARED_305185, sort_blocks=40, lane_bits=2, heavy_min=64),
    "11": SHARED_305185,                                    # sort_blocks=300 is out of range: ignored
    "12": dict(path="LARGE", c=16, K=16, nb=524288, lds_sort=0, sub=8),
    "12g": "not-supported",
    "13": dict(path="LARGE", K=26, nb=13312, lds_sort=1),
    "14": dict(path="LARGE", K=20, nb=81920, lds_sort=0),
    "15": dict(path="LARGE", tabled=3, own=1, nb=24576, bstride=1024, kout=24),
    "15g": "not-supported",
    "16": dict(path="SMALL", tabled=0),                     # per-window tables of another window than this size gets: not used
    "17": dict(path="SMALL", tabled=2),
    "18": dict(path="FIXED", tabled=2, Qf=5),
    "19": "invalid",
    "20": "invalid",
    "21": dict(path="LARGE", tabled=0, c=9, pstride=0),
    "22": dict(path="LARGE", sub=8),
    "23": dict(path="LARGE", sub=16),
    "24": "invalid",
    "25": "invalid",
    "26": "invalid",
    "27": "invalid",
    "28": "not-supported",
    "29": dict(K=37),
    "30": dict(path="LARGE", c=11, K=24),
}


@pytest.fixture(scope="module")
def shape_lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("msm_shape") / "msm_shape_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "vimz_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "msm_shape_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = {}
    for line in out.stdout.splitlines():
        head, _, rest = line.partition(": ")
        assert head.startswith("case ") and head[5:] not in lines, line
        lines[head[5:]] = rest
    return lines


def _fields(rest):
    words = rest.split()
    assert words[0] == "ok", rest
    out = {}
    for w in words[1:]:
        k, _, v = w.partition("=")
        out[k] = v if k == "path" else int(v)
    return out


def test_every_case_is_reported(shape_lines):
    assert set(shape_lines) == set(EXPECTED)


@pytest.mark.parametrize("case", sorted(EXPECTED, key=lambda c: (int(c.rstrip("g")), c)))
def test_shape_matches_the_launcher_it_replaced(shape_lines, case):
    want, got = EXPECTED[case], shape_lines[case]
    if isinstance(want, str):
        assert got == want
        return
    f = _fields(got)
    assert {k: f[k] for k in want} == want
    # the reduce's sums and the unit sum fit the pinned buffer
    assert f["kout"] + f["split_ones"] <= f["max_windows"] == 96
    assert f["sums"] == f["kout"] + f["split_ones"]


def test_no_small_switch_leaves_the_large_shape_alone(shape_lines):
    assert shape_lines["5"] == shape_lines["4"]
