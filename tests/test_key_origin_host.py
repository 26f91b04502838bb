"""The per-thread functions of k_spmv3_dict and k_origin_vec (vimz_amd/csrc/g16_key_origin_stage.hpp: spmv_dict_row, ko_expand, ko_unit, ko_h_scalar, ko_add) without a
GPU.

tests/native/key_origin_check.cpp, built with g++ -fsanitize=address,undefined and run directly, loops them over every thread of their grids under the kernels' guards on
heap blocks of the arrays' exact sizes — checking after every thread of the product that it wrote its own slot and no other, and every row against a naive dense product —
over the shapes the GPU test of the kernel runs (tests/_key_origin_ref.spmv_cases: n_c around a wave and a block, the paddings, rows empty and of 1, 64, 65 and 700
terms, a column named twice, the last column, coefficients 0, 1, r − 1) and the scalar builders' edges.  Here its words against Python integers."""
import os
import subprocess

import pytest

from tests import _key_origin_ref as O
from tests._pairing import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPMV = ("1/tight", "63/loose", "64/tight", "65/loose", "257/tight", "long_rows", "n_c_is_n")
MAX128 = O.MAX128


def vec_cases():
    rho = [0, 1, MAX128, 0x0123456789ABCDEFFEDCBA9876543210, 1 << 127, 77, MAX128 - 1]
    ninv = pow(64, -1, R)
    u = [(k * 0x9E3779B97F4A7C15F39CC0605CEDC835 + 5) % R for k in range(8)]
    u[7] = R - 1
    return {"expand/public": ("EXPAND", (7, 0, 3, ninv), rho), "expand/private": ("EXPAND", (7, 3, 7, ninv), rho), "expand/unscaled_all": ("EXPAND", (7, 0, 7, 1), rho),
            "expand/none": ("EXPAND", (7, 7, 7, 1), rho), "units/last_slot": ("UNITS", (5, 2, 8), u, [1, R - 1, MAX128]), "units/tail": ("UNITS", (2, 0, 8), u, [R - 1]),
            "hscalars/2": ("HSCALARS", (2,), [MAX128]), "hscalars/8": ("HSCALARS", (8,), rho), "add": ("ADD", (8,), u, [R - x if x else 0 for x in u[:4]] + [R - 1, 1, 0, 2])}


def vec_expected(case):
    what, sizes, x = case[0], case[1], case[2]
    if what == "EXPAND":
        count, lo, hi, scale = sizes
        return [x[i] * scale % R if lo <= i < hi else 0 for i in range(count)]
    if what == "UNITS":
        n_c, n_pub, _n = sizes
        return [(v + (case[3][i - n_c] if n_c <= i <= n_c + n_pub else 0)) % R for i, v in enumerate(x)]
    if what == "HSCALARS":
        return O.h_scalars(x, sizes[0])
    return [(a + b) % R for a, b in zip(x, case[3])]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("key_origin")
    exe, spec = d / "key_origin_check", d / "cases.txt"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "key_origin_check.cpp")])
    hx = lambda vals: " ".join(f"{int(v):x}" for v in vals)      # noqa: E731
    lines = []
    cases = O.spmv_cases()
    for name in SPMV:
        c = cases[name]
        mats = " ".join(f"{len(col)} {hx_dec(row_ptr)} {hx_dec(col)} {hx_dec(coef)}" for row_ptr, col, coef in c["mats"])
        lines.append(f"SPMV spmv/{name} {c['m']} {c['n_c']} {c['n']} {len(c['dict'])} {hx(c['dict'])} {hx(c['v'])} {mats}")
    for name, case in vec_cases().items():
        what, sizes = case[0], list(case[1])
        if what == "EXPAND":
            sizes[3] = f"{sizes[3]:x}"
        lines.append(f"{what} {name} {' '.join(str(s) for s in sizes)} " + " ".join(hx(v) for v in case[2:]))
    spec.write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(spec)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return {line.split()[0]: [int(w, 16) for w in line.split()[1:]] for line in out.stdout.splitlines()}


def hx_dec(vals):
    return " ".join(str(int(v)) for v in vals)


def test_every_case_is_reported(native):
    assert set(native) == {f"spmv/{n}" for n in SPMV} | set(vec_cases())


@pytest.mark.parametrize("name", SPMV)
def test_cpu_loop_of_the_product(native, name):
    case = O.spmv_cases()[name]
    want = O.spmv_expected(case)
    assert native[f"spmv/{name}"] == want[0] + want[1] + want[2]
    assert all(row == 0 for w in want for row in w[case["n_c"]:])


@pytest.mark.parametrize("name", sorted(vec_cases()))
def test_cpu_loop_of_the_scalar_builders(native, name):
    assert native[name] == vec_expected(vec_cases()[name])


def test_the_cases_hold_what_the_kernel_can_get_wrong():
    cases = O.spmv_cases()
    assert {c["n_c"] for c in cases.values()} >= {1, 63, 64, 65, 257}
    lengths = {b - a for c in cases.values() for row_ptr, _c, _k in c["mats"] for a, b in zip(row_ptr, row_ptr[1:])}
    assert {0, 1, 64, 65, 700} <= lengths
    assert any(c["n"] == c["n_c"] + 1 for c in cases.values()) and any(c["n"] > c["n_c"] + 1 for c in cases.values()) and any(c["n"] == c["n_c"] for c in cases.values())
    long = cases["long_rows"]
    assert any(c == long["m"] - 1 for c in long["mats"][0][1]) and {0, 1, R - 1} <= set(long["dict"]) and {0, MAX128, R - 1} <= set(long["v"])
    row_ptr, col, _k = long["mats"][0]
    assert any(col[a] == col[a + 1] for a, b in zip(row_ptr, row_ptr[1:]) if b - a >= 2)
    assert all(len(set(len(M[1]) for M in c["mats"])) > 1 for name, c in cases.items() if name != "1/tight" and name != "1/loose")      # three matrices of different shapes


def test_the_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "vimz_amd", "csrc", "g16_key_origin_stage.hpp")).read()
    assert "KO_BLOCK = 256;" in src and "KO_EXPAND = 0, KO_UNITS = 1, KO_H_SCALARS = 2, KO_ADD = 3" in src
