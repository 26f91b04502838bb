"""GPU half of tests/test_gpu_g16_kernels.py, a process of its own with VIMZ_HIP_LIBRARY=testing (`python -m tests._g16_kernels_gpu OUT.json`): the cases of
tests/_g16_ref.py through vimz_test_g16_domain / _fixed_mul / _g2_msm — the decider's own NTT, quotient, key-point and G2 MSM functions.  Vectors leave as the
hex of their little-endian words; nothing is judged here but the G2 bases the MSM cases are built from.  Test infrastructure."""
import ctypes as C
import json
import random
import sys
import time

import numpy as np

from tests import _g16_ref as G
from tests._pairing import G2, Q, R, g2_mul, g2_on_curve

MONT = 1 << 256
SPOT = 16                        # bases of the MSM pool compared with g2_mul


def to_words(vals):
    """ints below 2^256 -> (n, 4) uint64, little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def from_words(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def hex_of(arr):
    return np.ascontiguousarray(arr, dtype="<u8").tobytes().hex()


def hex_ints(h):
    raw = bytes.fromhex(h)
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def ints_hex(vals):
    """what hex_of gives for a vector that holds these integers"""
    return b"".join(int(v).to_bytes(32, "little") for v in vals).hex()


def main(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    lib = ctx.lib
    vp = C.c_void_p
    lib.vimz_test_g16_domain.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]
    lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    lib.vimz_test_g16_g2_msm.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp, vp]
    ptr = hip._ptr

    def domain(logn, what, a, b=None, c=None, form=_lib.FORM_CANONICAL):
        out = np.full((1 << logn, 4), 7, dtype=np.uint64)
        ctx._chk(lib.vimz_test_g16_domain(ctx.h, logn, what, ptr(a), ptr(b), ptr(c), form, ptr(out)))
        return out

    def fixed_mul(group, scalars):
        sc = to_words(scalars)
        out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
        ctx._chk(lib.vimz_test_g16_fixed_mul(ctx.h, group, ptr(sc), len(scalars), ptr(out)))
        return out

    def g2_msm_raw(bases, wires, m, form, idx, n=None):
        out = np.full(16, 7, dtype=np.uint64)
        rc = lib.vimz_test_g16_g2_msm(ctx.h, ptr(bases), len(idx) if n is None else n, ptr(wires), m, form, ptr(idx), ptr(out))
        return rc, out

    res = {"transform": {}, "quotient": {}, "fixed": {}, "msm": {}, "refused": {}}
    try:
        # ---- transforms and quotients
        for logn in G.TRANSFORM_LOGN:
            for name, v in G.transform_cases(logn).items():
                a = to_words(v)
                fwd = domain(logn, 0, a)
                res["transform"][f"{logn}/{name}"] = {"fwd": hex_of(fwd), "inv": hex_of(domain(logn, 1, a)), "coset": hex_of(domain(logn, 2, a)),
                                                      "inv_of_fwd": hex_of(domain(logn, 1, fwd))}
            for name, (a, b, c, _) in G.quotient_cases(logn).items():
                res["quotient"][f"{logn}/{name}"] = hex_of(domain(logn, 3, to_words(a), to_words(b), to_words(c)))
        # (the Montgomery form once: what the prover's vectors are in)
        a, b, c, _ = G.quotient_cases(3)["random"]
        mont = lambda v: to_words([x * MONT % R for x in v])      # noqa: E731
        res["quotient_montgomery/3"] = hex_of(domain(3, 3, mont(a), mont(b), mont(c), form=_lib.FORM_MONTGOMERY))
        one = to_words([1, 2])
        res["refused"]["logn_0"] = lib.vimz_test_g16_domain(ctx.h, 0, 0, ptr(one), None, None, 0, ptr(one.copy()))
        res["refused"]["logn_27"] = lib.vimz_test_g16_domain(ctx.h, 27, 0, ptr(one), None, None, 0, ptr(one.copy()))
        res["refused"]["not_reduced"] = lib.vimz_test_g16_domain(ctx.h, 1, 0, ptr(to_words([R, 0])), None, None, 0, ptr(one.copy()))
        # ---- fixed-base multiplication
        for group in (1, 2):
            for n in G.FIXED_N:
                res["fixed"][f"{group}/{n}"] = hex_of(fixed_mul(group, G.fixed_scalars(n)))
        # ---- the G2 MSM over bases k_i·G2 made by the kernel above, judged here: all on the curve, SPOT of them against g2_mul
        pool_k = G.msm_pool_scalars()
        pool = fixed_mul(2, pool_k)
        pool_pts = [G.g2_from_words(from_words(row)) for row in pool]
        res["pool_off_curve"] = [i for i, p in enumerate(pool_pts) if p is None or not g2_on_curve(p) or max(max(p[0]), max(p[1])) >= Q]
        spot = sorted({0, 1, G.MSM_POOL - 1} | set(random.Random("g16/msm/spot").sample(range(G.MSM_POOL), SPOT - 3)))
        res["pool_spot_wrong"] = [i for i in spot if pool_pts[i] != g2_mul(G2, pool_k[i])]
        res["pool_spot"] = spot
        neg = {}      # rows of −P_j

        def base_rows(bs):
            rows = np.zeros((len(bs), 16), dtype=np.uint64)
            for i, b in enumerate(bs):
                if b > 0:
                    rows[i] = pool[b - 1]
                elif b < 0:
                    if b not in neg:
                        neg[b] = to_words(G.g2_words(G.g2_neg(pool_pts[-b - 1]))).reshape(16)
                    rows[i] = neg[b]
            return rows

        def run_case(case):
            wires, idx = G.msm_layout(case)
            if case["form"] == _lib.FORM_MONTGOMERY:
                wires = [x * MONT % R for x in wires]
            rc, out = g2_msm_raw(base_rows(case["bases"]), to_words(wires), len(wires), case["form"], np.array(idx, dtype=np.uint32))
            ctx._chk(rc)
            return hex_of(out)

        for name, case in G.msm_cases().items():
            res["msm"][name] = run_case(case)
        res["msm_repeat"] = [run_case(G.msm_cases()[G.MSM_REPEAT]) for _ in range(2)]
        rows, w3, ix = base_rows([1, 2]), to_words([1, 2, 3]), np.array([0, 2], dtype=np.uint32)
        res["refused"]["msm_n_0"] = g2_msm_raw(rows, w3, 3, 0, ix, n=0)[0]
        res["refused"]["msm_n_above_m"] = g2_msm_raw(rows, w3, 1, 0, ix)[0]
        res["refused"]["msm_idx_not_below_m"] = g2_msm_raw(rows, w3, 3, 0, np.array([0, 3], dtype=np.uint32))[0]
        res["accepted"] = g2_msm_raw(rows, w3, 3, 0, ix)[0]
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"g16 kernels probe ok: {len(res['transform'])} transforms, {len(res['quotient'])} quotients, {len(res['msm'])} sums, {res['seconds']:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1])
