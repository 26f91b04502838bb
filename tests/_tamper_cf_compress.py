"""Body of tests/test_gpu_cf_compress.py::test_a_wrong_witness_still_compresses_and_is_rejected, run as a process of its own with VIMZ_HIP_LIBRARY=testing (the
hook that overwrites a prover's vectors, vimz_cf_poke, exists only in libvimz_hip_testing.so).  The prover does not judge its witness: with one element of a
running witness replaced vimz_cf_compress still returns a blob, and the verifier rejects exactly the argument that speaks about that witness.  The un-poked
proof of the same process is the control.  Test infrastructure."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests._oracle import from_limbs
    from tests.test_circuits import step_inputs
    from vimz_amd import _lib, folding, hip
    from vimz_amd.circuit import Circuit
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    c = Circuit.for_resolution("hash", "HD")
    n1 = 1 << (max(c.n_wires, c.n_constraints) + folding.CYCLEFOLD_ROOM - 1).bit_length()
    ck1 = ctx.bases_generate(_lib.CURVE_BN254_G1, n1)
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, folding.SECONDARY_KEY_LEN, b"ck-cyclefold")
    z0, inputs = step_inputs("hash")
    cf = hip.CycleFoldIVC(ctx, c, ck1, ck2, max_batch=4)
    try:
        cf.reset(z0)
        cf.fold(np.stack(inputs)[:3])
        assert cf.verify(3, z0) == 0
        control, _ = cf.compress()
        codes = {"control": cf.verify_compressed(control, 3, z0)}
        for name, which, side, what in (("cyclefold", 2, 1, hip.IX_RUNNING_Z), ("main", 0, 0, hip.IX_RUNNING_Z)):
            vec = from_limbs(cf.export(side, what))
            old = vec[1]
            cf.poke(which, 1, (old + 1) % _lib.MODULUS[side])
            blob, _ = cf.compress()                       # (no error: the prover does not judge the witness)
            assert len(blob) == len(control)
            codes[name] = cf.verify_compressed(blob, 3, z0)
            cf.poke(which, 1, old)
        again, _ = cf.compress()
        codes["restored"] = cf.verify_compressed(again, 3, z0)
        codes["restored_same_bytes"] = int(again.tobytes() == control.tobytes())
    finally:
        cf.close()
        ck1.free(); ck2.free()
        ctx.close()
    print("codes " + " ".join(f"{k}={v}" for k, v in codes.items()))


if __name__ == "__main__":
    main()
