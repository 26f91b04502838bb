"""TEST INFRASTRUCTURE ONLY.  The child process of tests/test_gpu_spartan_pub.py: runs the cases of tests/_spartan_pub_ref.py through the hooks
vimz_test_spartan_instance_pub / _pub_verify of libvimz_hip_testing.so (start it with VIMZ_HIP_LIBRARY=testing) and writes what came back as JSON.  The forged
arguments the product's verifier must reject are made here by the integer prover (CPU oracle for the group side); the comparison with the honest integer prover
happens in the test."""
import ctypes as C
import json
import sys
import time

import numpy as np

from tests import _oracle
from tests import _spartan_pub_ref as P
from tests import _spartan_ref as S
from tests._oracle import CURVE_SCALAR
from tests._spartan_kernels_gpu import Coo, point_words, to_words


def main(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    orc = _oracle.load()
    ctx = hip.Context(0)
    lib = ctx.lib
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    lib.vimz_test_spartan_instance.argtypes = [vp, C.c_int, sz, sz, vp, vp, vp, vp, vp, vp, vp, u32, C.c_char_p, vp, sz]
    lib.vimz_test_spartan_instance.restype = C.c_int64
    lib.vimz_test_spartan_instance_pub.argtypes = [vp, C.c_int, sz, sz, u32, vp, vp, vp, vp, vp, vp, vp, u32, C.c_char_p, vp, sz]
    lib.vimz_test_spartan_instance_pub.restype = C.c_int64
    lib.vimz_test_spartan_instance_pub_verify.argtypes = [vp, C.c_int, sz, sz, u32, vp, vp, vp, vp, vp, u32, C.c_char_p, vp, C.c_int, vp, sz]
    ptr = hip._ptr
    keys = {}
    res = {"case": {}, "refused": {}}

    def coos(c):
        keep, out = [], []
        for m in "ABC":
            trip = c[m]
            r, col = np.array([t[0] for t in trip], dtype=np.uint32), np.array([t[1] for t in trip], dtype=np.uint32)
            v = to_words([t[2] for t in trip])
            keep += [r, col, v]
            out.append(Coo(r.ctypes.data, col.ctypes.data, v.ctypes.data, len(trip)))
        return keep, out

    def prove(c, n_pub=None, n_w=None, old=False):
        keep, (A, B, Cm) = coos(c)
        Zw = to_words(c["Z"])
        Ew = to_words(c["E"]) if c["E"] is not None else None
        cap = 128 + S.argument_size(c)
        buf = np.full(cap // 8, 7, dtype=np.uint64)
        dg = to_words([c["digest"]])
        nw = c["n_w"] if n_w is None else n_w
        if old:
            n = lib.vimz_test_spartan_instance(ctx.h, c["cid"], c["n_c"], nw, C.byref(A), C.byref(B), C.byref(Cm), ptr(Zw), ptr(Ew), keys[c["cid"]].h, ptr(dg),
                                               c["side_tag"], P.LABEL, ptr(buf), cap)
        else:
            n = lib.vimz_test_spartan_instance_pub(ctx.h, c["cid"], c["n_c"], nw, c["n_pub"] if n_pub is None else n_pub, C.byref(A), C.byref(B), C.byref(Cm), ptr(Zw),
                                                   ptr(Ew), keys[c["cid"]].h, ptr(dg), c["side_tag"], P.LABEL, ptr(buf), cap)
        return int(n), buf

    def verify(c, blob, u, X, n_pub=None, n_w=None):
        """the instance (cW, cE of the blob; u, X as given) and the blob's argument through the product's verifier"""
        keep, (A, B, Cm) = coos(c)
        inst = np.concatenate([np.frombuffer(blob[:128], dtype="<u8").astype(np.uint64), to_words([u] + list(X)).reshape(-1)])
        words = np.frombuffer(blob[128:], dtype="<u8").astype(np.uint64)
        return int(lib.vimz_test_spartan_instance_pub_verify(ctx.h, c["cid"], c["n_c"], c["n_w"] if n_w is None else n_w, len(X) if n_pub is None else n_pub, C.byref(A),
                                                             C.byref(B), C.byref(Cm), keys[c["cid"]].h, ptr(to_words([c["digest"]])), c["side_tag"], P.LABEL, ptr(inst),
                                                             int(c["E"] is not None), ptr(words), words.size))

    try:
        for cid in (0, 1):
            keys[cid] = ctx.bases_upload(cid, point_words(S.key_points(cid)))
        for name in P.case_names():
            c = P.case(name)
            ps = S.FIELD[CURVE_SCALAR[c["cid"]]]
            n, buf = prove(c)
            if n != 128 + S.argument_size(c):
                ctx._chk(n if n < 0 else 0)
                raise AssertionError(f"{name}: {n} bytes, expected {128 + S.argument_size(c)}")
            blob = buf.tobytes()
            u, X = c["Z"][0], list(c["Z"][c["n_w"] - c["n_pub"]:])
            out = {"blob": blob.hex(), "verify": verify(c, blob, u, X), "u_plus_1": verify(c, blob, (u + 1) % ps, X), "x_plus_1": [], "forged": {}}
            for k in range(c["n_pub"]):
                Xb = list(X); Xb[k] = (Xb[k] + 1) % ps
                out["x_plus_1"].append(verify(c, blob, u, Xb))
            for i in P.forge_indices(c):
                inst, fb = P.prove(orc, c, forge=i)
                out["forged"][str(i)] = verify(c, fb, inst[2], inst[3])
            if c["n_pub"] == 2:
                n2, buf2 = prove(c, old=True)
                out["old_hook"] = buf2.tobytes().hex() if n2 == n else n2
            res["case"][name] = out
        # ---- refused shapes: no committed wire, no public element (both hooks)
        c = P.case("0/2x3x1/relaxed")
        blob = bytes.fromhex(res["case"]["0/2x3x1/relaxed"]["blob"])
        ref = res["refused"]
        ref["prove_n_w_is_n_pub_plus_1"] = prove(c, n_pub=2)[0]
        ref["prove_n_pub_0"] = prove(c, n_pub=0)[0]
        ref["verify_n_w_is_n_pub_plus_1"] = verify(c, blob, c["Z"][0], c["Z"][1:], n_pub=2)
        ref["verify_n_pub_0"] = verify(c, blob, c["Z"][0], [], n_pub=0)
        c7 = P.case("1/2x9x7/relaxed")
        ref["prove_n_w_8_n_pub_7"] = prove(c7, n_w=8)[0]
        n, buf = prove(c)
        res["accepted_after"] = {"rc": n, "same": buf.tobytes().hex() == res["case"]["0/2x3x1/relaxed"]["blob"]}
    finally:
        for kb in keys.values():
            kb.free()
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"spartan public-slot probe ok: {len(res['case'])} instances, {res['seconds']:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1])
