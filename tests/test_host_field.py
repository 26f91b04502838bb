"""Host-side field arithmetic of the library (the verifier circuits' witnesses are computed on the host with it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lazy_dot_product_equals_sum_of_products(tmp_path):
    exe = tmp_path / "fp_dot_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "vimz_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "fp_dot_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for f in ("BnFr", "BnFq", "PallasFp", "VestaFq"):
        assert f"{f}: 0 mismatches" in out.stdout


def test_lazily_reduced_coordinate_field_and_curve_formulas(tmp_path):
    """vimz_amd/csrc/fp29.hpp + ec.hpp compiled for the host: 9x29-bit lazy arithmetic == the canonical 8x32 arithmetic on every
    representative the formulas admit, and 12 000 random curve operations per curve (mixed / full additions, doublings, the
    doubling and cancellation branches) stay inside the documented bounds and equal the canonical computation."""
    exe = tmp_path / "fp29_lazy_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "vimz_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "fp29_lazy_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    for f in ("BnFr", "BnFq", "PallasFp", "VestaFq"):
        assert f"{f}: field 0 mismatches" in out.stdout
    for c in ("BnG1", "Grumpkin", "Pallas", "Vesta"):
        assert f"{c}: curve 0 mismatches" in out.stdout


def test_fp29_probe_on_the_host_matches_python_integers(tmp_path):
    """vimz_amd/csrc/fp29_probe.hpp compiled with g++ (the function the testing library's kernel calls, tests/test_gpu_fp29_probe.py): every operation
    of the lazily reduced field on raw operands — residues {0, 1, 2, p - 1, p - 2, (p - 1) / 2, 2^k - 1, 2^k, 2^k + 1} under every lift the operation's
    contract allows, the bound pairs at the limit (64, 1) ... (1, 64), limbs drawn from {0, 1, 2^28, 2^29 - 1}, all 256 top values of weak_reduce, the
    multiples of p around is_zero_mod, 20 000 random in-contract operands — against Python integers: value, limb normalisation and the bound fp29.hpp
    documents as an exact inequality.  This is also what validates the vectors and the reference themselves."""
    from tests import _fp29_ref as ref
    blocks = ref.all_blocks()
    assert len(blocks) == 4 * len(ref.OPS) and {b.op for b in blocks} == set(ref.OPS)
    outs = ref.run_host_probe(ref.build_host_probe(tmp_path), blocks, tmp_path)
    total = sum(ref.check_block(b, o) for b, o in zip(blocks, outs))
    assert total == sum(len(b) for b in blocks) and all(len(b) >= ref.RANDOM_PER_OP + 300 for b in blocks)
    # the limit pairs are among mul's operands, the 70 000-term sum's neighbourhood (2^261 - 1) among weak_reduce's
    for f in range(4):
        p = ref.MODULUS[f]
        mul = next(b for b in blocks if b.field == f and b.op == "mul")
        assert {(ref.bound_of(a, p), ref.bound_of(b, p)) for a, b, _, _ in mul.operands} >= set(ref.LIMIT_PAIRS)
        wr = next(b for b in blocks if b.field == f and b.op == "weak_reduce")
        assert {a >> 253 for a, _, _, _ in wr.operands} == set(range(256)) and (ref.TOP - 1, 0, 0, 0) in wr.operands


def test_fp29_probe_covers_every_sub_in_the_tree():
    """sub<K> has one compile-time constant K·p per instantiation: the probe must know every K the library's sources use."""
    from tests import _fp29_ref as ref
    used = ref.sub_instantiations_in_tree()
    assert used and used <= set(ref.SUB_K), f"sub<K> instantiated in vimz_amd/csrc but not in fp29_probe.hpp / tests/_fp29_ref.py: {sorted(used - set(ref.SUB_K))}"
    probe = open(os.path.join(ROOT, "vimz_amd", "csrc", "fp29_probe.hpp")).read()
    assert all(f"sub<{k}>" in probe for k in ref.SUB_K)
