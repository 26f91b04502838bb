#!/usr/bin/env python3
"""Times the compressed Nova + CycleFold proofs (vimz_cf_compress, vimz_cf_merged_compress) beside the Nova IVC's (vimz_ivc_compress,
vimz_ivc_merged_compress) on the same GPU in the same run: set-up, prove, verify and bytes of each.  A record, not a gate (profiles/cf_compress.txt).
usage: cf_compress_bench.py [transformation] [resolution] [rows]      (default: contrast HD 20; the merged proofs are of three segments)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import bench  # noqa: E402
from vimz_amd import folding, hip  # noqa: E402
from vimz_amd.distributed import fold_segments_merged  # noqa: E402


def timed_verify(fn):
    fn()                                  # (the verifier key's own set-up, first call only)
    t0 = time.time()
    code = fn()
    return code, time.time() - t0


def main():
    t = sys.argv[1] if len(sys.argv) > 1 else "contrast"
    res = sys.argv[2] if len(sys.argv) > 2 else "HD"
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    rows, z0 = bench.build_inputs(t, res)
    rows = np.stack(rows[:n])
    out = {"config": f"{t}_step_{res}", "rows": n, "segments_merged": 3, "kinds": {}}
    for backend, mode, one_cls, merged_cls in (("nova-snark", "ivc", hip.IVC, hip.MergedProof), ("sonobe", "cyclefold", hip.CycleFoldIVC, hip.CycleFoldMerged)):
        ctxs = [hip.Context(0) for _ in range(3)]
        circuit, params = folding.prepare_folding(ctxs[0], t, res, backend=backend)
        ck2 = params.secondary_key()
        batch = min(n, folding.default_batch(circuit))
        provers = [one_cls(c, circuit, params.ck, ck2, max_batch=batch) for c in ctxs]
        vk = one_cls(ctxs[0], circuit, params.ck, ck2, max_batch=1)
        try:
            one = provers[0]
            one.reset(z0); one.fold(rows)
            assert one.verify(n, z0) == 0
            blob, tc = one.compress()
            code, tv = timed_verify(lambda: vk.verify_compressed(blob, n, z0))
            info = one.info()
            out["kinds"][mode] = {"setup_s": tc["setup_s"], "prove_s": tc["prove_s"], "verify_s": tv, "bytes": int(len(blob)), "verify_code": code,
                                  "shape": {k: v for k, v in info.items() if k.endswith(("wires", "constraints"))}}
            _, tc2 = one.compress()
            out["kinds"][mode]["prove_again_s"] = tc2["prove_s"]
            mname = "merged" if mode == "ivc" else mode + "-merged"
            merged = fold_segments_merged(provers, rows, z0)
            try:
                assert merged.verify(n, z0) == 0
                mblob, tm = merged.compress()
                code, tv = timed_verify(lambda: merged_cls.verify_compressed(vk, mblob, n, z0))
                out["kinds"][mname] = {"setup_s": tm["setup_s"], "prove_s": tm["prove_s"], "verify_s": tv, "bytes": int(len(mblob)), "verify_code": code}
                _, tm2 = merged.compress()
                out["kinds"][mname]["prove_again_s"] = tm2["prove_s"]
            finally:
                merged.close()
        finally:
            for o in provers + [vk]:
                o.close()
            params.free()
            for c in ctxs:
                c.close()
    k = out["kinds"]
    out["ratios"] = {"cyclefold / ivc prove": k["cyclefold"]["prove_s"] / k["ivc"]["prove_s"],
                     "cyclefold-merged / merged prove": k["cyclefold-merged"]["prove_s"] / k["merged"]["prove_s"],
                     "cyclefold / cyclefold-merged prove": k["cyclefold"]["prove_s"] / k["cyclefold-merged"]["prove_s"],
                     "cyclefold / ivc bytes": k["cyclefold"]["bytes"] / k["ivc"]["bytes"],
                     "cyclefold-merged / merged bytes": k["cyclefold-merged"]["bytes"] / k["merged"]["bytes"]}
    for name, v in k.items():
        print(f"{name:18s} set-up {v['setup_s']:.3f} s  prove {v['prove_s']:.3f} s (again {v['prove_again_s']:.3f} s)  verify {v['verify_s']:.3f} s  {v['bytes']} bytes  code {v['verify_code']}")
    for name, v in out["ratios"].items():
        print(f"ratio {name}: {v:.2f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
