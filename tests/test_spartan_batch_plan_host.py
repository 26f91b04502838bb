"""The GPU-free pieces of the batched compressed-proof verifier (vimz_amd/csrc/spartan_batch_plan.hpp: the half-tables' per-thread body, the index map and mask of
k_svec_accum, the unrolled coefficients of an opening's equation, the chunk plan) on the CPU: tests/native/spartan_batch_check.cpp, built with
g++ -fsanitize=address,undefined and run directly, checks each against the definition it stands for on both scalar fields and ends without a sanitizer report.
No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = tmp_path_factory.mktemp("spartan_batch_plan") / "spartan_batch_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "vimz_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "spartan_batch_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.splitlines()[-1] == "done bad=0" and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-4000:]
    return {ln.split()[0]: {k: int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])} for ln in out.stdout.splitlines()[:-1]}


def test_every_loop_ran_and_found_nothing(native):
    assert set(native) == {"fr/tables", "fq/tables", "index_map", "fr/unroll", "fq/unroll", "chunks"}
    for name, t in native.items():
        assert t["runs"] > 0 and t["bad"] == 0, name
    assert native["fr/tables"]["runs"] == 14 and native["chunks"]["runs"] == 101 * 41
