"""Measures vimz_decider_verify_batch against the single verifier and writes profiles/decider_verify_batch.txt:  python tools/decider_verify_bench.py [--sizes 1,64,1024,16384]
[--rounds 5] [--out profiles/decider_verify_batch.txt].  Needs an MI355X.

Workload: the light hash decider's key, ONE valid proof (2 steps) repeated n times.  Per n, the wall time of the C calls alone (arrays prepared before):
  (a) n calls of vimz_decider_verify_key spread over 16 host threads — the only way before the batch entry;
  (b) vimz_decider_verify_batch with ctx = NULL (the host path);
  (c) vimz_decider_verify_batch on the device, with its `seconds` split.
One warm-up, then `rounds` rounds: median and range.  One extra line: the largest n <= 1024 with a single bad proof (negated C) in the middle — the fallback's cost."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,16384")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decider_verify_batch.txt"))
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    from tests.test_circuits import step_inputs
    from tests._pairing import Q
    from vimz_amd import _lib, calldata, hip
    from vimz_amd.circuit import Circuit
    ctx = hip.Context(0)
    srs, kzg_vk = hip.kzg_setup(ctx, 36000)
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
    cf = hip.CycleFoldIVC(ctx, Circuit.for_resolution("hash", "HD"), srs, ck2, max_batch=2)
    z0, inputs = step_inputs("hash")
    cf.reset(z0); cf.fold(np.stack(inputs[:2]))
    dec = hip.Decider(cf, kzg_vk=kzg_vk, light=True)
    _, d = calldata.decider_calldata(dec)
    kw = np.ascontiguousarray(dec.key_words(), dtype=np.uint64)
    lz = len(d["z0"])
    one = {"z0": hip._zlimbs(d["z0"], lz), "zi": hip._zlimbs(d["z_i"], lz), "w": hip._zlimbs(d["words"], 25)}
    bad_words = list(d["words"]); bad_words[16] = Q - bad_words[16]
    bad_w = hip._zlimbs(bad_words, 25)
    lib, vp = ctx.lib, C.c_void_p
    lib.vimz_decider_verify_key.argtypes = [vp, C.c_size_t, C.c_uint64, vp, vp, C.c_uint32, vp, C.POINTER(C.c_uint32)]
    lib.vimz_decider_verify_batch.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_size_t, vp, vp, vp, vp, C.c_size_t, vp, C.POINTER(C.c_double)]
    p = hip._ptr

    def single_calls(n):
        def work(count):
            res = C.c_uint32(0)
            for _ in range(count):
                assert lib.vimz_decider_verify_key(p(kw), kw.size, d["steps"], p(one["z0"]), p(one["zi"]), lz, p(one["w"]), C.byref(res)) == 0 and res.value == 0
        counts = [n // THREADS + (1 if t < n % THREADS else 0) for t in range(THREADS)]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(THREADS) as ex:
            list(ex.map(work, [c for c in counts if c]))
        return time.perf_counter() - t0, None

    def batch(n, handle, bad_at=None):
        steps = np.full(n, d["steps"], dtype=np.uint64)
        z0a, zia, wa = np.tile(one["z0"], (n, 1)), np.tile(one["zi"], (n, 1)), np.tile(one["w"], (n, 1))
        if bad_at is not None:
            wa[25 * bad_at:25 * (bad_at + 1)] = bad_w
        res = np.zeros(n, dtype=np.uint32)
        sec = (C.c_double * 6)()

        def call(_n):
            t0 = time.perf_counter()
            assert lib.vimz_decider_verify_batch(handle, p(kw), kw.size, lz, n, p(steps), p(z0a), p(zia), p(wa), 0, p(res), sec) == 0
            dt = time.perf_counter() - t0
            want = np.zeros(n, dtype=np.uint32)
            if bad_at is not None:
                want[bad_at] = 8
            assert (res == want).all()
            return dt, [float(x) for x in sec]
        return call

    def measure(fn, n):
        fn(n)
        runs = [fn(n) for _ in range(args.rounds)]
        ts = sorted(r[0] for r in runs)
        mid = sorted(runs, key=lambda r: r[0])[len(runs) // 2]
        return statistics.median(ts), ts[0], ts[-1], mid[1]

    lines = [f"vimz_decider_verify_batch against the single verifier — light hash decider's key, one valid 2-step proof repeated n times; {args.rounds} rounds after a warm-up,",
             "median (min .. max) seconds of the C calls alone.  (a) n calls of vimz_decider_verify_key over 16 host threads; (b) the batch with ctx = NULL; (c) the batch on the",
             "device, with the median round's split: parse + host / per-proof stage / Miller loops / chunk products / fallback.", ""]
    fmt = lambda m: f"{m[0]:.4f} ({m[1]:.4f} .. {m[2]:.4f})"      # noqa: E731
    try:
        for n in sizes:
            a, b, c = measure(single_calls, n), measure(batch(n, None), n), measure(batch(n, ctx.h), n)
            lines.append(f"n = {n:6d}   (a) {fmt(a)}   (b) {fmt(b)}   (c) {fmt(c)}   split " + " / ".join(f"{x:.4f}" for x in c[3][:5]))
            print(lines[-1], flush=True)
        n = max(x for x in sizes if x <= 1024)
        b, c = measure(batch(n, None, bad_at=n // 2), n), measure(batch(n, ctx.h, bad_at=n // 2), n)
        lines.append(f"n = {n:6d} with ONE bad proof (negated C) at index {n // 2}: (b) {fmt(b)}   (c) {fmt(c)}   split " + " / ".join(f"{x:.4f}" for x in c[3][:5]))
        print(lines[-1], flush=True)
    finally:
        dec.close(); cf.close(); srs.free(); ck2.free(); ctx.close()
    with open(args.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
