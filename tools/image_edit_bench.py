"""Image edits: one vimz_image_edit call per transformation at HD, 4K and 8K (the edited pixels, the packed source and the packed target, as
the prover's input needs them), median milliseconds with the library's upload / kernels / download split — beside the host editor
(vimz_amd.image_editor.build_input, single-threaded numpy) on the same image.  Every GPU result is checked against the host's.  The 4K / 8K
images are the reference's img2 upscaled by nearest neighbour, as tests/_data.config_rows builds them.

    python tools/image_edit_bench.py [--reps 5] [--host-reps 1] [--out profiles/image_edit_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _data  # noqa: E402
from vimz_amd import hip  # noqa: E402
from vimz_amd import image_editor as ie  # noqa: E402

SCALE = {"HD": 1, "4K": 3, "8K": 6}
OPS = ("contrast", "brightness", "grayscale", "resize", "crop", "sharpness", "blur", "redact", "hash")


def params(op, res):
    if op in ("contrast", "brightness"):
        return {"factor": 1.4}
    if op == "crop":
        return {"x": 200, "y": 100, "crop_size": "SD" if res == "HD" else "FHD"}
    if op == "resize":
        return {"resize_to": {"HD": (640, 480), "4K": (1920, 1080), "8K": (3840, 2160)}[res]}
    return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--resolutions", default="HD,4K,8K")
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--sha", default=None, help="the commit the tree is (default: git rev-parse HEAD)")
    a = ap.parse_args()
    sha = a.sha
    if not sha:
        try:
            sha = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "?"
        except OSError:
            sha = "?"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    with hip.Context(0) as ctx:
        say(f"# tools/image_edit_bench.py at {sha}  device: {ctx.device_info()['name']}  reps {a.reps} (median)  host reps {a.host_reps} (median)")
        say("# res  op          MB_in  MB_out  gpu_ms  upload_ms  kernels_ms  download_ms   host_ms  host/gpu")
        results = []
        for res in a.resolutions.split(","):
            k = SCALE[res]
            img = np.ascontiguousarray(np.repeat(np.repeat(_data.load_image("img2"), k, axis=0), k, axis=1))
            for op in a.ops.split(","):
                p = params(op, res)
                d = ie._edit_desc(op, **p)
                d["pixels"] = img
                ctx.image_edit([d])                                # (warm-up: code objects, the grow-only buffer)
                tot, up, ker, down = [], [], [], []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    r = ctx.image_edit([d])[0]
                    tot.append((time.perf_counter() - t) * 1e3)
                    pr = ctx.image_edit_last_profile()
                    up.append(pr["upload"])
                    ker.append(pr["kernels"])
                    down.append(pr["download"])
                host = []
                for _ in range(a.host_reps):
                    t = time.perf_counter()
                    want = ie.build_input(op, img, **p)
                    host.append((time.perf_counter() - t) * 1e3)
                got = ie._as_input(op, p, img.shape, r)
                assert np.array_equal(got["original"], want["original"]), (res, op)
                assert (want["transformed"] is None and got["transformed"] is None) or np.array_equal(got["transformed"], want["transformed"]), (res, op)
                mb_out = sum(v.nbytes for v in r.values() if v is not None) / 1e6
                g, u, kk, dd, h = (float(np.median(v)) for v in (tot, up, ker, down, host))
                results.append({"res": res, "op": op, "mb_in": img.nbytes / 1e6, "mb_out": mb_out, "gpu_ms": g, "upload_ms": u, "kernels_ms": kk,
                                "download_ms": dd, "host_ms": h, "host_over_gpu": h / g})
                say(f"{res:>4}  {op:<10}  {img.nbytes / 1e6:5.0f}  {mb_out:6.0f}  {g:6.1f}  {u:9.1f}  {kk:10.2f}  {dd:11.1f}  {h:8.0f}  {h / g:8.1f}")
        say("# gpu_ms: the whole call (Python request -> edited pixels, packed source and packed target on the host); upload / kernels / download: "
            "vimz_image_edit_last_profile; host: vimz_amd.image_editor.build_input (packed source and target) on one host thread")
        say(json.dumps({"sha": sha, "results": results}))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
