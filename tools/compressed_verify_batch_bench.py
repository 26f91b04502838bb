#!/usr/bin/env python3
"""Times vimz_cf_verify_compressed_batch / vimz_ivc_verify_compressed_batch against a loop of the single verifier on the same blobs, in the same run, and writes
profiles/compressed_verify_batch.txt.  A record, not a gate.  One compressed proof of `rows` folded rows is made once and repeated n times (every member is
verified in full: the batch holds no cache across members).
usage: compressed_verify_batch_bench.py [--kind cyclefold|ivc] [--transformation contrast] [--resolution HD] [--rows 4] [--sizes 1,16,64,256] [--out FILE]"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import bench  # noqa: E402
from vimz_amd import folding, hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="cyclefold", choices=("cyclefold", "ivc"))
    ap.add_argument("--transformation", default="contrast")
    ap.add_argument("--resolution", default="HD")
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--sizes", default="1,16,64,256")
    ap.add_argument("--out", default=__file__.rsplit("/tools/", 1)[0] + "/profiles/compressed_verify_batch.txt")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    rows, z0 = bench.build_inputs(a.transformation, a.resolution)
    rows = np.stack(rows[:a.rows])
    ctx = hip.Context(0)
    cls = hip.CycleFoldIVC if a.kind == "cyclefold" else hip.IVC
    circuit, params = folding.prepare_folding(ctx, a.transformation, a.resolution, backend="sonobe" if a.kind == "cyclefold" else "nova-snark")
    ck2 = params.secondary_key()
    prover = cls(ctx, circuit, params.ck, ck2, max_batch=min(a.rows, folding.default_batch(circuit)))
    vk = cls(ctx, circuit, params.ck, ck2, max_batch=1)
    lines, record = [], {"kind": a.kind, "config": f"{a.transformation}_step_{a.resolution}", "rows": a.rows, "sizes": {}}
    try:
        prover.reset(z0); prover.fold(rows)
        blob, _ = prover.compress()
        assert vk.verify_compressed(blob, a.rows, z0) == 0          # (the verifier key's own set-up: outside every timing)
        assert vk.verify_compressed_batch([blob], [a.rows], [z0])[0] == [0]
        info = prover.info()
        shape = {k: v for k, v in info.items() if k.endswith(("wires", "constraints"))}
        for n in sizes:
            t0 = time.time()
            codes = [vk.verify_compressed(blob, a.rows, z0) for _ in range(n)]
            t_single = time.time() - t0
            t0 = time.time()
            words, sec = vk.verify_compressed_batch([blob] * n, [a.rows] * n, [z0] * n)
            t_batch = time.time() - t0
            assert codes == [0] * n == words, (codes, words)
            record["sizes"][str(n)] = {"single_loop_s": t_single, "batch_s": t_batch, "seconds": sec}
            lines.append(f"n = {n:4d}   single-verifier loop {t_single:8.3f} s ({1e3 * t_single / n:7.2f} ms a proof)   batch {t_batch:8.3f} s ({1e3 * t_batch / n:7.2f} ms a proof)"
                         f"   ratio {t_single / t_batch:6.2f}")
            lines.append("           batch split: " + "  ".join(f"{k[:-2]} {v:.4f}" for k, v in sec.items()))
        # one tampered member in a chunk of 32: the fallback, measured
        if max(sizes) >= 32:
            bad = np.array(blob, dtype=np.uint8).copy(); bad[len(bad) - 32] ^= 1
            blobs = [blob] * 31 + [bad]
            t0 = time.time()
            words, sec = vk.verify_compressed_batch(blobs, [a.rows] * 32, [z0] * 32)
            t_bad = time.time() - t0
            assert words[:31] == [0] * 31 and words[31] != 0
            record["one_bad_in_32"] = {"batch_s": t_bad, "seconds": sec}
            lines.append(f"one tampered member in a chunk of 32: {t_bad:.3f} s, of which fallback {sec['fallback_s']:.3f} s (32 single verifications)")
        faster = [n for n in sizes if record["sizes"][str(n)]["single_loop_s"] < record["sizes"][str(n)]["batch_s"]]
        lines.append("the single call is the faster one at n = " + (", ".join(str(n) for n in faster) if faster else "none of the sizes measured"))
    finally:
        prover.close(); vk.close(); params.free(); ctx.close()
    head = [f"vimz_{'cf' if a.kind == 'cyclefold' else 'ivc'}_verify_compressed_batch against a loop of the single verifier — {record['config']}, one compressed \"{a.kind}\" proof of {a.rows} rows",
            f"repeated n times, default chunk (32), wall-clock of the Python call, one run; shape {json.dumps(shape)}; blob {len(blob)} bytes", ""]
    text = "\n".join(head + lines) + "\n\n" + json.dumps(record) + "\n"
    with open(a.out, "w") as fp:
        fp.write(text)
    print(text)


if __name__ == "__main__":
    main()
