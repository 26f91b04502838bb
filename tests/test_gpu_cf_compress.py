"""Compressed Nova + CycleFold proofs on the GPU, one chain (vimz_cf_compress / vimz_cf_verify_compressed) and merged segments (vimz_cf_merged_compress /
vimz_cf_verify_merged_compressed): the product's verifier on a second prover object accepts, the independent verifier of tests/_spartan_cf.py accepts, both
reject another statement and tampered blobs, a blob of the other kind is malformed, and a prover whose witness was overwritten still writes a blob that the
verifier rejects in the argument about that witness.  `hash` at HD, the ten rows of step_inputs("hash")."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _spartan_cf
from tests.test_circuits import step_inputs
from vimz_amd import _lib, folding
from vimz_amd.circuit import Circuit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pow2(n):
    return 1 << (n - 1).bit_length()


@pytest.fixture(scope="module")
def ctx():
    from vimz_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def setup(ctx):
    """keys, the step circuit, a verifier key (a CycleFoldIVC that never folds) and the key prefixes the independent verifier reads, their lengths from info()"""
    from vimz_amd import hip
    c = Circuit.for_resolution("hash", "HD")
    ck1 = ctx.bases_generate(_lib.CURVE_BN254_G1, _pow2(max(c.n_wires, c.n_constraints) + folding.CYCLEFOLD_ROOM))
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, folding.SECONDARY_KEY_LEN, b"ck-cyclefold")
    vk = hip.CycleFoldIVC(ctx, c, ck1, ck2, max_batch=1)
    info = vk.info()
    n1, n2 = _pow2(max(info["main_wires"], info["main_constraints"])), _pow2(max(info["cyclefold_wires"], info["cyclefold_constraints"]))
    assert info["cyclefold_io"] == 7 and n1 <= ck1.n and n2 <= ck2.n
    s = {"circuit": c, "ck1": ck1, "ck2": ck2, "vk": vk, "info": info, "n1": n1, "n2": n2, "key1": ck1.download(0, n1), "key2": ck2.download(0, n2)}
    yield s
    vk.close()
    ck1.free(); ck2.free()


@pytest.fixture(scope="module")
def chain(ctx, setup):
    """ten folded rows, their compressed proof and what the statement is"""
    from vimz_amd import hip
    z0, inputs = step_inputs("hash")
    cf = hip.CycleFoldIVC(ctx, setup["circuit"], setup["ck1"], setup["ck2"], max_batch=4)
    cf.reset(z0)
    cf.fold(np.stack(inputs))
    assert cf.verify(10, z0) == 0
    blob, t = cf.compress()
    yield {"cf": cf, "blob": blob, "t": t, "z0": z0, "zn": cf.state()[0], "inputs": np.stack(inputs)}
    cf.close()


@pytest.fixture(scope="module")
def merged(ctx, setup):
    """segments of 4, 3 and 3 rows folded by three provers and merged; the compressed proof of the merged object"""
    from vimz_amd import hip
    from vimz_amd.distributed import fold_segments_merged, segment_bounds
    z0, inputs = step_inputs("hash")
    assert [hi - lo for lo, hi in segment_bounds(10, 3)] == [4, 3, 3]
    ctxs = [ctx, hip.Context(0), hip.Context(0)]
    cfs = [hip.CycleFoldIVC(c, setup["circuit"], setup["ck1"], setup["ck2"], max_batch=4) for c in ctxs]
    m = fold_segments_merged(cfs, np.stack(inputs), z0)
    assert m.verify(10, z0) == 0 and m.info()["segments"] == 3
    blob, t = m.compress()
    yield {"m": m, "blob": blob, "z0": z0, "zn": m.state()[1]}
    m.close()
    for o in cfs + ctxs[1:]:
        o.close()


def _lib_fn(ctx, name, restype=None):
    import ctypes as C
    fn = getattr(ctx.lib, name)
    fn.argtypes = [C.c_void_p]
    fn.restype = C.c_size_t if restype is None else restype
    return fn


def _chain_offsets(info):
    """byte offsets of: an instance coordinate, a sum-check message, a claimed evaluation, an IPA point (all of the first argument); the last is the blob's end"""
    s1, t1 = (info["main_constraints"] - 1).bit_length(), (info["main_wires"] - 1).bit_length()
    inst = 8 + 8 * info["len_z"]
    args = inst + 4 * (7 + 4 + 12)
    return {"instance coordinate": 8 * inst, "sum-check message": 8 * (args + 4), "claimed evaluation": 8 * (args + 12 * s1), "IPA point": 8 * (args + 12 * s1 + 16 + 8 * t1 + 4)}


def test_one_chain_compresses_and_a_second_prover_object_verifies(ctx, setup, chain):
    vk, blob, z0 = setup["vk"], chain["blob"], chain["z0"]
    assert len(blob) == _lib_fn(ctx, "vimz_cf_compressed_size")(chain["cf"].h) == _lib_fn(ctx, "vimz_cf_compressed_size")(vk.h)
    assert len(blob) < 64 * 1024
    assert vk.verify_compressed(blob, 10, z0) == 0
    assert vk.state()[1] == 0                                                        # (the verifier key's folding state is not touched)
    assert vk.verify_compressed(blob, 9, z0) & 4096
    assert vk.verify_compressed(blob, 10, [z0[0] + 1]) & (4096 | 1) == (4096 | 1)
    places = _chain_offsets(setup["info"])
    places["final scalar"] = len(blob) - 32
    assert len(places) == 5 and all(0 <= off < len(blob) for off in places.values())
    for what, off in places.items():
        bad = blob.copy()
        bad[off] ^= 1
        assert vk.verify_compressed(bad, 10, z0) != 0, f"a flipped bit in the {what} was accepted"
    # a prover with nothing folded has nothing to compress
    with pytest.raises(_lib.VimzError) as e:
        vk.compress()
    assert e.value.code == _lib.ERR_INVALID


def test_independent_verifier_on_one_chain(setup, chain, oracle):
    vk, blob, z0 = setup["vk"], chain["blob"], chain["z0"]
    args = (setup["key1"], setup["key2"])
    failed, zn = _spartan_cf.verify_chain(oracle, vk, blob, 10, z0, *args)
    assert failed == [] and zn == chain["zn"]
    assert _spartan_cf.verify_chain(oracle, vk, blob, 11, z0, *args)[0] != []
    bad = blob.copy()
    bad[_chain_offsets(setup["info"])["claimed evaluation"]] ^= 1
    assert _spartan_cf.verify_chain(oracle, vk, bad, 10, z0, *args)[0] != []


def test_merged_segments_compress_and_a_fresh_verifier_key_verifies(ctx, setup, merged):
    from vimz_amd import hip
    vk, blob, z0 = setup["vk"], merged["blob"], merged["z0"]
    assert len(blob) == _lib_fn(ctx, "vimz_cf_merged_compressed_size")(merged["m"].h)
    verify = lambda b, n, z: hip.CycleFoldMerged.verify_compressed(vk, b, n, z)      # noqa: E731
    assert verify(blob, 10, z0) == 0
    assert verify(blob, 9, z0) & 4096
    assert verify(blob, 10, [z0[0] + 1]) & 4096
    rw = int(np.frombuffer(blob[8:16].tobytes(), dtype="<u8")[0])
    for what, off in (("record word", 8 * (2 + 8 + 1 + 1 + 4)), ("argument word", 8 * (2 + rw + 4))):          # (the first segment's z_start; round 0's s2)
        bad = blob.copy()
        bad[off] ^= 1
        assert verify(bad, 10, z0) != 0, f"a flipped bit in a {what} was accepted"
    bad = blob.copy()
    bad[8 * (2 + 1)] ^= 1                                                             # the records' own count of segments: framing
    assert verify(bad, 10, z0) == 8192


def test_a_blob_of_the_other_kind_is_malformed(setup, chain, merged):
    from vimz_amd import hip
    vk = setup["vk"]
    assert hip.CycleFoldMerged.verify_compressed(vk, chain["blob"], 10, chain["z0"]) == 8192
    assert vk.verify_compressed(merged["blob"], 10, merged["z0"]) == 8192
    assert vk.verify_compressed(chain["blob"][:-8], 10, chain["z0"]) == 8192
    assert hip.CycleFoldMerged.verify_compressed(vk, merged["blob"][:-8], 10, merged["z0"]) == 8192
    magics = {int(np.frombuffer(b[:8].tobytes(), dtype="<u8")[0]) for b in (chain["blob"], merged["blob"])}
    assert len(magics) == 2 and magics.isdisjoint({0x314E5343565A, 0x31474D43565A}) and magics == {k for k, v in folding.COMPRESSED_MAGIC.items() if v.startswith("cyclefold")}


def test_independent_verifier_on_merged_segments(setup, merged, oracle):
    vk, blob, z0 = setup["vk"], merged["blob"], merged["z0"]
    args = (setup["key1"], setup["key2"])
    failed, zn = _spartan_cf.verify_merged(oracle, vk, blob, 10, z0, *args)
    assert failed == [] and zn == merged["zn"]
    assert _spartan_cf.verify_merged(oracle, vk, blob, 11, z0, *args)[0] != []
    bad = blob.copy()
    bad[len(blob) - 32] ^= 1
    assert _spartan_cf.verify_merged(oracle, vk, bad, 10, z0, *args)[0] != []


def test_a_short_commitment_key_is_refused(ctx, setup):
    from vimz_amd import hip
    # enough generators to fold (one for every wire and row), fewer than the padded shape
    n_short = max(setup["info"]["main_wires"], setup["info"]["main_constraints"])
    assert n_short < setup["n1"]
    short = ctx.bases_generate(_lib.CURVE_BN254_G1, n_short)
    try:
        cf = hip.CycleFoldIVC(ctx, setup["circuit"], short, setup["ck2"], max_batch=1)
        try:
            z0, inputs = step_inputs("hash")
            cf.reset(z0); cf.fold(np.stack(inputs)[:1])
            with pytest.raises(_lib.VimzError) as e:
                cf.compress()
            assert e.value.code == _lib.ERR_INVALID and "commitment key is shorter" in str(e.value)
        finally:
            cf.close()
    finally:
        short.free()


def test_a_wrong_witness_still_compresses_and_is_rejected():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_tamper_cf_compress.py")], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    codes = dict(kv.split("=") for kv in [ln for ln in r.stdout.splitlines() if ln.startswith("codes ")][-1].split()[1:])
    codes = {k: int(v) for k, v in codes.items()}
    assert codes["control"] == 0 and codes["restored"] == 0 and codes["restored_same_bytes"] == 1
    assert codes["cyclefold"] & 8, codes          # bit 3: the argument for cfU_n
    assert codes["main"] & 4, codes               # bit 2: the argument for U_n


@pytest.mark.parametrize("segments", [1, 3])
def test_through_folding(ctx, segments):
    """prepare_folding -> fold_input(mode="cyclefold") -> compress_proof -> verify_compressed_proof"""
    circuit, params = folding.prepare_folding(ctx, "hash", "HD", backend="sonobe")
    z0, inputs = step_inputs("hash")
    proof = None
    try:
        proof = folding.fold_input(params, np.stack(inputs), z0, max_batch=4, mode="cyclefold", segments=segments)
        assert proof.mode == ("cyclefold" if segments == 1 else "cyclefold-merged")
        folding.verify_folded_proof(proof, params, 10, z0)
        blob, t = folding.compress_proof(params, proof)
        vk = proof.prover if segments == 1 else proof.verifier_key
        folding.verify_compressed_proof(vk, blob, 10, z0)
        folding.verify_compressed_proof(vk, blob.tobytes(), 10, z0)
        with pytest.raises(_lib.VimzError):
            folding.verify_compressed_proof(vk, blob, 9, z0)
        assert set(t) == {"setup_s", "prove_s"}
    finally:
        if proof is not None:
            proof.close()
        params.free()


def test_folding_on_gives_a_proof_of_the_longer_statement_only(setup, chain):
    vk, cf, z0 = setup["vk"], chain["cf"], chain["z0"]
    cf.fold(chain["inputs"][:3])
    blob13, _ = cf.compress()
    assert vk.verify_compressed(blob13, 13, z0) == 0 and vk.verify_compressed(chain["blob"], 10, z0) == 0
    assert vk.verify_compressed(blob13, 10, z0) != 0 and vk.verify_compressed(chain["blob"], 13, z0) != 0
