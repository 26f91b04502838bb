"""Image hashes: milliseconds per image on the GPU (vimz_image_hash: the unit digests in one launch, the running chain on the host) at HD, 4K
and 8K, one image per call and batches of 2 and 8 — beside the same hash on 16 host threads (the CPU oracle's ArrayHasher per row over a
thread pool, then its Poseidon chain; test infrastructure, as bench.py's CPU baseline).  The 4K / 8K images are the reference's img2 upscaled
by nearest neighbour, as tests/_data.config_rows builds them.

    python tools/image_hash_bench.py [--reps 3] [--host-threads 16] [--out profiles/image_hash_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _data  # noqa: E402
from tests import _image_hash_oracle as iho  # noqa: E402
from tests import _oracle  # noqa: E402
from vimz_amd import hip, image_hasher  # noqa: E402

SCALE = {"HD": 1, "4K": 3, "8K": 6}


def image(res, variant=0):
    k = SCALE[res]
    img = np.repeat(np.repeat(_data.load_image("img2"), k, axis=0), k, axis=1)
    if variant:
        img = img.copy()
        img[variant % img.shape[0], 0, 0] ^= 1        # (distinct images in a batch)
    return np.ascontiguousarray(img)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--batches", default="1,2,8")
    ap.add_argument("--resolutions", default="HD,4K,8K")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sha", default=None, help="the commit the tree is (default: git rev-parse HEAD)")
    a = ap.parse_args()
    sha = a.sha
    if not sha:
        try:
            sha = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "?"
        except OSError:
            sha = "?"
    orc = _oracle.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    with hip.Context(0) as ctx:
        say(f"# tools/image_hash_bench.py at {sha}  device: {ctx.device_info()['name']}  reps {a.reps} (median)  host threads {a.host_threads}")
        say("# res  batch  gpu_ms/img  digests_ms/img  chain_ms/img  host_ms/img  host/gpu")
        results = []
        pool = ThreadPoolExecutor(a.host_threads)
        for res in a.resolutions.split(","):
            imgs = [image(res, v) for v in range(max(int(b) for b in a.batches.split(",")))]
            t = time.perf_counter()
            want = iho.image_hash(orc, {"image": imgs[0]}, pool)       # host: one image, its rows over the pool, then the chain
            host_ms = (time.perf_counter() - t) * 1e3
            image_hasher.image_hashes(ctx, imgs[:1])                   # (warm-up: tables, code objects)
            for b in [int(x) for x in a.batches.split(",")]:
                tot, dig, chn = [], [], []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    got = image_hasher.image_hashes(ctx, imgs[:b])
                    tot.append((time.perf_counter() - t) * 1e3)
                    p = ctx.image_hash_last_profile()
                    dig.append(p["digests"])
                    chn.append(p["chain"])
                assert got[0] == want, (res, b)
                g, d, c = (float(np.median(v)) / b for v in (tot, dig, chn))
                r = {"res": res, "batch": b, "gpu_ms_per_image": g, "digests_ms_per_image": d, "chain_ms_per_image": c, "host_ms_per_image": host_ms,
                     "host_over_gpu": host_ms / g}
                results.append(r)
                say(f"{res:>4}  {b:>5}  {g:10.1f}  {d:14.1f}  {c:12.1f}  {host_ms:11.1f}  {host_ms / g:8.1f}")
        say("# gpu_ms: the whole call (Python request -> hashes) over the batch, per image; digests / chain: vimz_image_hash_last_profile (digests = "
            "uploads + kernel + download; chain = the host's PairHasher chains, one image per thread); host: one image on the host threads")
        say(json.dumps({"sha": sha, "results": results}))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
