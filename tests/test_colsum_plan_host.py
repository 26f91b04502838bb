"""The column sums and the h query of a set-up from a powers-of-tau string (vimz_amd/csrc/g16_powers.hip: k_col_runs, k_point_diff) without a GPU.

tests/native/colsum_plan_check.cpp, built with g++ -fsanitize=address,undefined and run directly, makes the host plan (vimz_amd/csrc/g16_colsum_plan.hpp) of every
case of tests/_g16_powers_ref.colsum_cases(), asserts the plan's invariants (every non-zero entry in exactly one run; no run over 1 024 entries; a run of one
column and one magnitude; a column's slots side by side; one final partial per column), loops the functions the kernels call with their thread index
(g16_point_stage.hpp: colsum_run, pt_diff) over every thread of every level in G1, and compares with plain double-and-add sums — a failure of any of these is its
exit status.  Here: its outputs against [colsum_expected]G on Python integers (the special columns and SPOT others of every case: g1_mul takes 80 ms), and the
plan it prints — the bookkeeping alone — evaluated on SCALARS against colsum_expected, every column.  The h query at n = 2 and 4."""
import os
import random
import subprocess

import pytest

from tests import _g16_powers_ref as W
from tests._decider_powers_gpu import G2_CASES
from tests._pairing import G1, R, g1_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CASES = W.colsum_cases()
CASES = {**REF_CASES, "own/long": (2, "long")}
SPOT = 6
FINAL = 1 << 31
HQ_TAU, HQ_DELTA = 0x1234567890ABCDEF1234567, 0x7654321FEDCBA9876543
HQ = {"hq/2": (2, HQ_DELTA, None), "hq/4": (4, HQ_DELTA, None), "hq/4/one": (4, 1, None), "hq/4/identity": (4, HQ_DELTA, 5), "hq/4/identity_low": (4, HQ_DELTA, 1)}      # n, delta, the index of an identity among the inputs: 5 a minuend P[j + n], 1 a subtrahend P[j]


def hq_scalars(n, hole):
    s = [pow(HQ_TAU, k, R) for k in range(2 * n - 1)]
    if hole is not None:
        s[hole] = 0
    return s


def hq_expected(n, delta, hole):
    s, dinv = hq_scalars(n, hole), pow(delta, -1, R)
    return [(s[j + n] - s[j]) * dinv % R for j in range(n - 1)]


def long_case():
    """beyond the reference's cases: ONE magnitude in more than COL_CHUNK entries of a column (coefficients 1 and r − 1 alike), so that level 0 cuts a group"""
    base = W.colsum_case(1, 1)
    n_rows = base["n_rows"]
    row_ptr, col, coef = [0], [], []
    for r in range(n_rows):
        if r < W.COL_CHUNK + 6:
            col.append(0); coef.append(r % 2)
        if r % 100 == 0:
            col.append(1); coef.append(2)
        row_ptr.append(len(col))
    return {"n_rows": n_rows, "n_cols": 2, "csr": (row_ptr, col, coef), "dict": base["dict"], "scalars": base["scalars"]}


def the_case(name):
    return long_case() if name == "own/long" else W.colsum_case(*CASES[name])


def case_text(name):
    c = the_case(name)
    row_ptr, col, coef = c["csr"]
    hx = lambda v: " ".join(f"{x:x}" for x in v)      # noqa: E731
    nums = lambda v: " ".join(str(x) for x in v)      # noqa: E731
    return (f"CASE {name} {c['n_rows']} {c['n_cols']} {len(c['dict'])}\nROWPTR {nums(row_ptr)}\nCOL {nums(col)}\nCOEF {nums(coef)}\n"
            f"DICT {hx(c['dict'])}\nSCALARS {hx(c['scalars'])}\n")


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("colsum_plan")
    exe, spec = d / "colsum_plan_check", d / "cases.txt"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "colsum_plan_check.cpp")])
    text = "".join(case_text(name) for name in CASES)
    text += "".join(f"HQ {name} {n} {pow(delta, -1, R):x} " + " ".join(f"{x:x}" for x in hq_scalars(n, hole)) + "\n" for name, (n, delta, hole) in HQ.items())
    spec.write_text(text)
    out = subprocess.run([str(exe), str(spec)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = {}
    for line in out.stdout.splitlines():
        tag, name, *words = line.split()
        case = res.setdefault(name, {"levels": []})
        if tag == "OUT":
            case["out"] = [int(w, 16) for w in words]
        elif tag == "MAGS":
            case["mags"] = [int(w, 16) for w in words]
        elif tag == "ENTRIES":
            case["entries"] = [int(w) for w in words]
        else:
            assert tag == "LEVEL" and int(words[0]) == len(case["levels"])
            v = [int(w) for w in words[2:]]
            case["levels"].append({"n_partials": int(words[1]), "runs": [tuple(v[i:i + 5]) for i in range(0, len(v), 5)]})
    return res


def point(s):
    p = g1_mul(G1, s % R)
    return [0, 0] if p is None else [p[0], p[1]]


def test_every_case_is_reported(native):
    assert set(native) == set(CASES) | set(HQ)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_loop_of_the_kernels_functions(native, name):
    case = the_case(name)
    want, got = W.colsum_expected(case), native[name]["out"]
    n = case["n_cols"]
    assert len(got) == 2 * n
    spot = set(range(min(n, 12))) | set(random.Random("colsum/spot/" + name).sample(range(n), min(n, SPOT)))
    for j in sorted(spot):
        assert got[2 * j:2 * j + 2] == point(want[j]), f"{name}: column {j}"
    for j in range(n):
        assert (got[2 * j:2 * j + 2] == [0, 0]) == (want[j] == 0), f"{name}: column {j}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_evaluated_on_scalars_is_the_column_sums(native, name):
    case = the_case(name)
    plan, s = native[name], case["scalars"]
    out, prev = [0] * case["n_cols"], None
    for k, level in enumerate(plan["levels"]):
        cur = [None] * level["n_partials"]
        for off, length, mag, bits, dst in level["runs"]:
            assert 1 <= length <= W.COL_CHUNK
            if k == 0:
                assert plan["mags"][mag].bit_length() == bits and 2 * plan["mags"][mag] < R
                total = sum(-s[e >> 1] if e & 1 else s[e >> 1] for e in plan["entries"][off:off + length]) * plan["mags"][mag] % R
            else:
                assert (mag, bits) == (0, 1)
                total = sum(prev[off:off + length]) % R
            if dst & FINAL:
                out[dst & ~FINAL] = total
            else:
                assert cur[dst] is None
                cur[dst] = total
        assert None not in cur
        prev = cur
    assert prev == []
    assert out == W.colsum_expected(case)
    # what the cases are to reach: a column over one chunk needs a second level; runs hold one magnitude, so the mixed cases make many
    if CASES[name][1] == "mixed" and case["n_cols"] > 5:
        assert len(plan["levels"]) >= 2 and max(r[1] for r in plan["levels"][0]["runs"]) <= W.COL_CHUNK
    if name == "own/long":
        assert sorted(r[1] for r in plan["levels"][0]["runs"]) == [6, 11, W.COL_CHUNK] and len(plan["levels"]) == 2
    if CASES[name][1] == "empty":
        assert plan["levels"] == [{"n_partials": 0, "runs": []}]


@pytest.mark.parametrize("name", sorted(HQ))
def test_h_query_on_the_cpu(native, name):
    n, delta, hole = HQ[name]
    want = hq_expected(n, delta, hole)
    got = native[name]["out"]
    assert len(got) == 2 * (n - 1)
    for j in range(n - 1):
        assert got[2 * j:2 * j + 2] == point(want[j]), f"{name}: output {j}"


def test_chunk_is_the_reference_s():
    src = open(os.path.join(ROOT, "vimz_amd", "csrc", "g16_colsum_plan.hpp")).read()
    assert f"COLSUM_CHUNK = {W.COL_CHUNK};" in src


def test_the_cases_hold_what_they_are_meant_to():
    assert set(REF_CASES) == {"1/mixed", "63/mixed", "64/mixed", "65/mixed", "1/0", "1/1", "1/31", "1/32", "1/33", "64/empty"} and set(G2_CASES) <= set(CASES)
    case = W.colsum_case(65, "mixed")
    row_ptr, col, coef = case["csr"]
    lengths = [col.count(j) for j in range(12)]
    assert lengths[:7] == [31, 32, 33, 0, 1, W.COL_CHUNK + 1, W.COL_CHUNK] and lengths[7:] == [2, 2, 3, 3, 3]
    want = W.colsum_expected(case)
    s, d = case["scalars"], case["dict"]
    assert want[7] == 2 * s[0] % R and want[8] == 0 and want[9] == s[5] and want[11] == 3 * s[0] % R and want[3] == 0      # doubling, cancelling, cancel-then-third, thrice
    assert 0 in s and {1, R - 1, 0, (R + 1) // 2, (R - 1) // 2} <= set(d) and W.colsum_expected(W.colsum_case(64, "empty")) == [0] * 64
