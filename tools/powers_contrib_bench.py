"""What profiles/powers_contrib.txt records: vimz_powers_contribute and vimz_powers_verify_contributions on the prefix of a string a decider of domain n = 2^LOGN
reads (n points of tau_g2, alpha_g1, beta_g1, 2n − 1 of tau_g1), and beside them, in the same process, the existing transform over n points of G1
(vimz_powers_lagrange: logn·n/2 multiplications of the same kind — the per-multiplication yardstick) and the same contribution looped on host threads over a 2^14
slice (tools/powers_contrib_host_loop.cpp, built here with g++ when it is not there), scaled to the string's 5n − 1 points of G1.

    VIMZ_HIP_LIBRARY=testing python tools/powers_contrib_bench.py LOGN [--reps R] [--out FILE.json]

One warm-up call of each, then R calls, every one listed with its median and range; host clocks around work that ends in a stream synchronise (the library's own
seconds[]).  The string is [s]G of known scalars made by the fixed-base hook of the testing library; secrets come from the OS.  No time is a pass or fail."""
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
NAMES = ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")
TAU, ALPHA, BETA = 0x2545F4914F6CDD1D0123456789ABCDEF, 0xFEDCBA987654321, 0x55AA55AA55AA77
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
HOST_SLICE, HOST_THREADS = 1 << 14, 16


def host_loop(reps):
    """seconds of `reps` runs of the host-thread loop over HOST_SLICE points"""
    exe = os.path.join(ROOT, "vimz_amd", "csrc", "build", "powers_contrib_host_loop")
    src = os.path.join(ROOT, "tools", "powers_contrib_host_loop.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O3", "-mbmi2", "-madx", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "vimz_amd", "csrc"), "-o", exe, src])
    out = subprocess.run([exe, str(HOST_SLICE), str(HOST_THREADS), str(reps)], capture_output=True, text=True, check=True, timeout=600)
    return [float(x) for x in out.stdout.split()]


def spread(xs):
    return {"all": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", type=int)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this tool with VIMZ_HIP_LIBRARY=testing: the string is made by the fixed-base hook"
    n = 1 << args.logn
    res = {"logn": args.logn, "n_pow": n, "n_tau_g1": 2 * n - 1, "g1_points": 5 * n - 1, "g2_points": n, "reps": args.reps}
    ctx = hip.Context(0)
    try:
        t0 = time.time()
        pw = [1] * (2 * n - 1)
        for k in range(1, len(pw)):
            pw[k] = pw[k - 1] * TAU % R
        scalars = {"tau_g1": pw, "tau_g2": pw[:n], "alpha_g1": [ALPHA * x % R for x in pw[:n]], "beta_g1": [BETA * x % R for x in pw[:n]], "beta_g2": [BETA]}
        ctx.lib.vimz_test_g16_fixed_mul.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        canon = {}
        for name in NAMES:
            group = 2 if name.endswith("g2") else 1
            words = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in scalars[name]), dtype="<u8").astype(np.uint64)
            canon[name] = np.zeros((len(scalars[name]), 8 * group), dtype=np.uint64)
            ctx._chk(ctx.lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(words), len(scalars[name]), hip._ptr(canon[name])))
        # into the file's Montgomery form, as iden3.read_ptau hands a string over (plain integers: this is set-up, not measured)
        def montgomery(a):
            raw = a.tobytes()
            return np.frombuffer(b"".join((int.from_bytes(raw[i:i + 32], "little") * (1 << 256) % Q).to_bytes(32, "little") for i in range(0, len(raw), 32)),
                                 dtype="<u8").astype(np.uint64).reshape(a.shape)
        origin = {name: montgomery(a) for name, a in canon.items()}
        origin["power"] = args.logn
        res["string_seconds"] = round(time.time() - t0, 1)
        contribute, verify, transform = [], [], []
        for rep in range(args.reps + 1):                       # (the first round warms every call up and is kept apart)
            sec = []
            out, rec = hip.contribute_powers(ctx, origin, seconds=sec)
            contribute.append(list(sec))
            sec = []
            res["verdict"] = hip.verify_powers_contributions(ctx, origin, out, rec, seconds=sec)
            verify.append(list(sec))
            sec = []
            hip.powers_lagrange(ctx, 1, origin["tau_g1"][:n], args.logn, form=_lib.FORM_MONTGOMERY, seconds=sec)
            transform.append(list(sec))
        res["warm_up"] = {"contribute": contribute[0], "verify": verify[0], "transform": transform[0]}
        res["contribute"] = {k: spread([c[i] for c in contribute[1:]]) for i, k in enumerate(("host", "device", "total"))}
        res["verify"] = {k: spread([v[i] for v in verify[1:]]) for i, k in enumerate(("points", "knowledge", "string"))}
        res["transform_g1"] = {k: spread([t[i] for t in transform[1:]]) for i, k in enumerate(("host", "device"))}
        res["transform_multiplications"] = args.logn * n // 2 + n
        res["contribute_multiplications"] = {"g1": 5 * n - 1, "g2": n}
    finally:
        ctx.close()
    loop = host_loop(args.reps + 1)
    res["host_loop"] = {"points": HOST_SLICE, "threads": HOST_THREADS, "warm_up": loop[0], "seconds": spread(loop[1:]),
                        "scaled_to_g1_points": round(statistics.median(loop[1:]) * (5 * n - 1) / HOST_SLICE, 2)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
