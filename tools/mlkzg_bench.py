"""What profiles/mlkzg_open.txt records: the multilinear KZG opening (vimz_mlkzg_open) of a vector of 2^logn random elements under a KZG SRS of that length — the
size of contrast HD's running vectors at the default 19 —, its four phases as the library reports them, the host verifier (vimz_mlkzg_verify) on the proof, and in
the same run vimz_kzg_open, the univariate opening of the same vector at one point.

    python tools/mlkzg_bench.py [--logn L] [--reps R] [--out FILE]

One warm-up round, then R rounds, every one listed with its median and range; all times are the wall clock around the call (each ends in a stream synchronise or
runs on the host).  No time is a pass or fail."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def spread(xs):
    return {"all": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=19)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    from vimz_amd import _lib, hip
    n = 1 << args.logn
    rng = np.random.default_rng(19)
    host = rng.integers(0, 1 << 61, size=(n, 4), dtype=np.uint64)                      # below r: the top limb has 61 bits, r's 62
    point = [int(x) for x in rng.integers(1, 1 << 62, size=args.logn)]
    ctx = hip.Context(0)
    res = {"logn": args.logn, "n": n, "reps": args.reps, "device": ctx.device_info()["name"]}
    try:
        t0 = time.perf_counter()
        srs, vk = hip.kzg_setup(ctx, n)
        res["kzg_setup_seconds"] = round(time.perf_counter() - t0, 3)
        vec = ctx.vec_from_host(_lib.FIELD_BN254_FR, host)
        timings = {"open": [], "verify": [], "kzg_open": [], **{p: [] for p in hip.MLKZG_PHASES}}
        for _ in range(args.reps + 1):                                                 # (the first round warms every call up and is kept apart)
            sec = {}
            t0 = time.perf_counter()
            comm, ev, proof = ctx.mlkzg_open(srs, vec, point, seconds=sec)
            t1 = time.perf_counter()
            verdict = hip.mlkzg_verify(vk, comm, point, ev, proof)
            t2 = time.perf_counter()
            ctx.kzg_open(srs, vec, point[0])
            t3 = time.perf_counter()
            assert verdict == 0, verdict
            timings["open"].append(t1 - t0); timings["verify"].append(t2 - t1); timings["kzg_open"].append(t3 - t2)
            for p in hip.MLKZG_PHASES:
                timings[p].append(sec[p])
        res["proof_bytes"] = int(proof.size) * 8
        res["warm_up"] = {k: round(v[0], 4) for k, v in timings.items()}
        res["seconds"] = {k: spread(v[1:]) for k, v in timings.items()}
        vec.free(); srs.free()
    finally:
        ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
