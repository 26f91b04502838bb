"""The per-thread functions of the multilinear KZG opening's kernels and its host verifier on the CPU (vimz_amd/csrc/mlkzg_stage.hpp, mlkzg_verify.hpp):
tests/native/mlkzg_check.cpp, built with g++ -fsanitize=address,undefined and run directly, loops them over every thread index at the sizes on each side of the
chunk, block and cross-block boundaries against a naive Horner, a naive division and the fold's definition, makes proofs out of those loops with a tau it knows and
runs the verifier and the parser over heap blocks of exact size.  The run must end without a sanitizer report, its proofs must be tests/_mlkzg_ref.py's word for
word, and its verdicts the expected ones.  No GPU; nothing here is loaded into Python."""
import os
import subprocess

import pytest

from tests import _mlkzg_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mlkzg") / "mlkzg_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "vimz_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "mlkzg_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "done"
    return dict(line.split(" ", 1) for line in lines[:-1])


def test_every_stage_was_compared_at_every_size(native):
    block, chunk = (int(t) for t in native["shape"].split())
    bc = block * chunk
    for n in (1, 2, chunk - 1, chunk, chunk + 1, bc - 1, bc, bc + 1, 2 * bc + 3):
        assert native[f"stage/eval3_divide/{n}"] == "ok"
    big = bc.bit_length()
    assert 1 << big > bc >= 1 << (big - 1)
    for logn in (1, 2, 3, big):
        for kind in range(3):
            assert native[f"stage/fold_batch/{logn}/{kind}"] == "ok"


@pytest.mark.parametrize("logn", (1, 2, 3, 5))
def test_the_loops_proofs_are_the_reference_s(native, logn):
    for n in sorted({1, (1 << logn) - 1, 1 << logn}):
        pr = M.prove(0x5555aaaa7 + logn, [1000 * logn + 3 * i + 1 for i in range(n)], logn, [7 * logn + 11 * k + 2 for k in range(logn)])
        assert [int(w, 16) for w in native[f"proof/{logn}/{n}"].split()] == pr["proof"], n
        assert native[f"verdict/{logn}/{n}"] == "0"


def test_the_verifier_s_verdicts(native):
    assert {k: native[k] for k in native if k.startswith("verdict/") and not k[8].isdigit()} == {
        "verdict/short": str(M.MALFORMED), "verdict/fold": str(M.FOLD), "verdict/pairing": str(M.PAIRING), "verdict/off_curve": str(M.OFF_CURVE),
        "verdict/element_r": str(M.MALFORMED), "verdict/coordinate_q": str(M.MALFORMED)}
    assert native["parse/logn_0"] == "0"
