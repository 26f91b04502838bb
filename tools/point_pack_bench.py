"""What profiles/point_pack.txt records: packing and unpacking (vimz_decider_key_pack / _unpack, vimz_points_pack / _unpack) of the light hash decider's key (domain
2^18; tests/_key_contrib_gpu.DeciderBench makes it) and of the prefix of a string that decider's set-up reads (n points of tau_g2, alpha_g1, beta_g1, 2n − 1 of
tau_g1), and beside them the same per-thread functions looped on 16 host threads over a slice (tools/point_pack_host_loop.cpp, built here with g++ when it is not
there), scaled to the same point counts.

    VIMZ_HIP_LIBRARY=testing python tools/point_pack_bench.py [--reps R] [--out FILE.json] [--full]

One warm-up round, then R rounds, every one listed with its median and range.  The key calls are timed by the wall clock around the C call (they end in a stream
synchronise); the point calls by the library's own seconds[] = {host, device with copies}, whose device share is reported.  --full: the full decider of contrast HD
instead of the light hash decider, the key alone (no string prefix).  No time is a pass or fail."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
HOST_SLICE, HOST_THREADS = {1: 1 << 16, 2: 1 << 15}, 16


def host_loop(group, reps):
    """[(pack seconds, unpack seconds)] of `reps` runs of the host-thread loop over HOST_SLICE[group] points"""
    exe = os.path.join(ROOT, "vimz_amd", "csrc", "build", "point_pack_host_loop")
    src = os.path.join(ROOT, "tools", "point_pack_host_loop.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O3", "-mbmi2", "-madx", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "vimz_amd", "csrc"), "-o", exe, src])
    out = subprocess.run([exe, str(group), str(HOST_SLICE[group]), str(HOST_THREADS), str(reps)], capture_output=True, text=True, check=True, timeout=600)
    return [tuple(float(x) for x in line.split()) for line in out.stdout.splitlines()]


def spread(xs):
    return {"all": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--full", action="store_true")
    args = ap.parse_args()
    from tests import _key_contrib_gpu as kg
    from tests import _point_pack_ref as ref
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this tool with VIMZ_HIP_LIBRARY=testing: the key is made by the trapdoor set-up hook"
    ctx, fixed_mul = kg.open_context()
    res = {"reps": args.reps, "decider": "full, contrast HD" if args.full else "light, hash HD"}
    try:
        bench = kg.DeciderBench(ctx, fixed_mul, "contrast" if args.full else "hash", light=not args.full)
        try:
            d0 = bench.trapdoor_decider(kg.DELTA)
            info = d0.info()
            key = d0.save_key()
            d0.close()
        finally:
            bench.close()
        L = ref.runs(info["wires"], info["public_inputs"], info["domain"])
        res.update({"domain": info["domain"], "key_bytes": int(key.size), "g1_points": L["n_g1"], "g2_points": L["n_g2"]})
        vp = C.c_void_p
        for name in ("vimz_decider_key_pack", "vimz_decider_key_unpack"):
            getattr(ctx.lib, name).argtypes, getattr(ctx.lib, name).restype = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint32), vp], C.c_int64
        packed = np.zeros(ref.packed_size(key.size), dtype=np.uint8)
        back = np.zeros(key.size, dtype=np.uint8)
        res["packed_key_bytes"] = int(packed.size)
        result, first = C.c_uint32(0), np.zeros(2, dtype=np.uint64)
        words = np.ascontiguousarray(key).view(np.uint64)
        runs = {"key_g1_run": (1, words[L["off_g1"]:L["off_g2"]].reshape(-1, 8)), "key_g2_run": (2, words[L["off_g2"]:L["words"]].reshape(-1, 16))}
        # the string's prefix for that domain, canonical words: [tau^k]G made by the fixed-base hook
        n = info["domain"]
        if not args.full:                                      # (the full decider's 2^22 prefix is left out: the key alone is measured there)
            pw = [1] * (2 * n - 1)
            for k in range(1, len(pw)):
                pw[k] = pw[k - 1] * kg.TAU % R
            runs["string_tau_g1"] = (1, fixed_mul(1, pw))
            runs["string_alpha_g1"] = (1, fixed_mul(1, [kg.ALPHA * x % R for x in pw[:n]]))
            runs["string_beta_g1"] = (1, fixed_mul(1, [kg.BETA * x % R for x in pw[:n]]))
            runs["string_tau_g2"] = (2, fixed_mul(2, pw[:n]))
        timings = {"key_pack_wall": [], "key_unpack_wall": []}
        timings.update({f"{name}/{way}/{part}": [] for name in runs for way in ("pack", "unpack") for part in ("host", "device")})
        for rep in range(args.reps + 1):                       # (the first round warms every call up and is kept apart)
            t0 = time.perf_counter()
            got = ctx.lib.vimz_decider_key_pack(ctx.h, hip._ptr(key), key.size, hip._ptr(packed), packed.size, C.byref(result), hip._ptr(first))
            t1 = time.perf_counter()
            assert got == packed.size and not result.value
            got = ctx.lib.vimz_decider_key_unpack(ctx.h, hip._ptr(packed), packed.size, hip._ptr(back), back.size, C.byref(result), hip._ptr(first))
            t2 = time.perf_counter()
            assert got == back.size and not result.value
            timings["key_pack_wall"].append(t1 - t0); timings["key_unpack_wall"].append(t2 - t1)
            for name, (group, pts) in runs.items():
                sec_p, sec_u = [], []
                pk = hip.pack_points(ctx, group, pts, seconds=sec_p)
                un = hip.unpack_points(ctx, group, pk, seconds=sec_u)
                if rep == 0:
                    assert np.array_equal(un, pts), name
                for way, sec in (("pack", sec_p), ("unpack", sec_u)):
                    timings[f"{name}/{way}/host"].append(sec[0]); timings[f"{name}/{way}/device"].append(sec[1])
        res["round_trip"] = bool(np.array_equal(back, key))
        res["warm_up"] = {k: round(v[0], 4) for k, v in timings.items()}
        res["seconds"] = {k: spread(v[1:]) for k, v in timings.items()}
        res["points"] = {name: int(pts.shape[0]) for name, (_g, pts) in runs.items()}
        res["device_share"] = {f"{name}/{way}": round(statistics.median(timings[f"{name}/{way}/device"][1:]) /
                                                     (statistics.median(timings[f"{name}/{way}/device"][1:]) + statistics.median(timings[f"{name}/{way}/host"][1:])), 3)
                               for name in runs for way in ("pack", "unpack")}
    finally:
        ctx.close()
    res["host_loop"] = {}
    for group in (1, 2):
        loop = host_loop(group, args.reps + 1)
        total = res["g1_points"] if group == 1 else res["g2_points"]
        res["host_loop"][f"g{group}"] = {"points": HOST_SLICE[group], "threads": HOST_THREADS, "warm_up": list(loop[0]), "pack_seconds": spread([x[0] for x in loop[1:]]),
                                        "unpack_seconds": spread([x[1] for x in loop[1:]]),
                                        "scaled_to_the_key's_points": {"pack": round(statistics.median([x[0] for x in loop[1:]]) * total / HOST_SLICE[group], 3),
                                                                      "unpack": round(statistics.median([x[1] for x in loop[1:]]) * total / HOST_SLICE[group], 3)}}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
