"""The framing of the two compressed Nova + CycleFold proofs as a verifier meets them — untrusted words (vimz_amd/csrc/cf_compressed_parse.hpp: header, exact
sizes, the records' framing, every bound later indexing relies on) — on the CPU: tests/native/cf_compressed_parse_check.cpp, built with
g++ -fsanitize=address,undefined and run directly, loops it over structurally valid blobs of both kinds, every truncation length and every single-word garbling
of the header and the records' framing, each input in a heap block of exactly its size.  Every input ends in "malformed" or a clean parse whose ranges are all
read, and the program ends without a sanitizer report.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("chain", "merged1", "merged2")


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cf_compressed_parse") / "cf_compressed_parse_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "cf_compressed_parse_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.splitlines()[-1].startswith("done ") and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-4000:]
    return {ln.split()[0]: {k: int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])} for ln in out.stdout.splitlines()[:-1]}


def test_every_loop_is_reported_and_every_input_ends_one_way_or_the_other(native):
    assert set(native) == {f"{k}/{loop}" for k in KINDS for loop in ("whole", "truncated", "longer", "garbled", "other_shape")} | {"cross/kinds"}
    for name, t in native.items():
        assert t["inputs"] > 0 and t["clean"] + t["malformed"] == t["inputs"], name


@pytest.mark.parametrize("kind", KINDS)
def test_only_a_whole_blob_for_this_circuit_parses(native, kind):
    assert native[f"{kind}/whole"] == {"inputs": 1, "clean": 1, "malformed": 0}
    for loop in ("truncated", "longer", "other_shape"):
        assert native[f"{kind}/{loop}"]["clean"] == 0, loop
    assert native[f"{kind}/truncated"]["inputs"] > 300          # every length from nothing up to one word short
    g = native[f"{kind}/garbled"]
    # what stays clean under a garbled word carries no framing: the step counts (16 values each at most) and, with two runs, a second run that starts at another segment
    assert g["malformed"] > 7 * g["clean"] and g["clean"] <= 16 * (1 if kind == "chain" else 3) + (16 if kind == "merged2" else 0)


def test_one_kind_is_malformed_for_the_other(native):
    assert native["cross/kinds"] == {"inputs": 2, "clean": 0, "malformed": 2}
