"""Body of tests/test_gpu_fp29_probe.py, run as a process of its own with VIMZ_HIP_LIBRARY=testing: the vectors of tests/_fp29_ref.py through
vimz_test_fp29_probe on the device, checked against the integer reference and, limb for limb, against the host build of the same function.
usage: _fp29_probe_gpu.py WORKDIR.  Test infrastructure."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(workdir):
    from tests import _fp29_ref as ref
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    blocks = ref.all_blocks()
    host = ref.run_host_probe(ref.build_host_probe(workdir), blocks, workdir)
    ctx = hip.Context(0)
    vp = C.c_void_p
    ctx.lib.vimz_test_fp29_probe.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_size_t]
    total = 0
    try:
        for b, h in zip(blocks, host):
            arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in b.arrays()]
            out = np.full((len(b), ref.WORDS), 0xffffffff, dtype=np.uint32)
            ctx._chk(ctx.lib.vimz_test_fp29_probe(ctx.h, b.field, ref.OPS[b.op], *[a.ctypes.data for a in arrs], out.ctypes.data, len(b)))
            total += ref.check_block(b, out, where="device")
            diff = np.nonzero((out != h).any(axis=1))[0]
            assert diff.size == 0, (f"device and host differ: {ref.FIELDS[b.field]} {b.op}, {diff.size} cases, first {int(diff[0])}: operands "
                                    f"{[hex(x) for x in b.operands[int(diff[0])]]} device {[hex(int(x)) for x in out[diff[0]]]} host {[hex(int(x)) for x in h[diff[0]]]}")
        # an operation the probe does not know is refused, not run
        z = np.zeros((1, ref.WORDS), dtype=np.uint32)
        assert ctx.lib.vimz_test_fp29_probe(ctx.h, 0, 108, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1) == _lib.ERR_INVALID
    finally:
        ctx.close()
    print(f"fp29 probe ok: {len(blocks)} blocks, {total} cases, at least {min(len(b) for b in blocks)} a block")


if __name__ == "__main__":
    main(sys.argv[1])
