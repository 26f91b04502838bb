"""GPU half of tests/test_gpu_msm_rows.py, a process of its own with VIMZ_HIP_LIBRARY=testing (`python -m tests._msm_rows_gpu OUT.json`): groups of rows
through vimz_test_msm_rows (msm_launch_rows + the grouped unit sums), every row alone through vimz_msm, one row through the CPU oracle.  Test infrastructure."""
import ctypes as C
import json
import random
import sys

import numpy as np

P = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001      # BN254 Fr
N = 33000                      # just above MSM_SMALL_MAX = 30 720: the sort / accumulate / combine / reduce pipeline
STRIDE = N + 137               # the rows lie further apart than they are long; what lies between them is dense and must not be read
N_ONES = 20001                 # prefix of every row whose unit sum rides along (the producer's S_1)
KINDS = ("zero", "one", "repeat", "random", "neg_small", "ones40", "random2", "bytes")
GROUPS = {1: (5,), 2: (2, 0), 3: (1, 3, 4), 8: (0, 1, 2, 3, 4, 5, 6, 7)}      # rows (indices into KINDS) of the group of each size
CALLS = 2
ORACLE_ROW = 3


def row(kind):
    rng = random.Random(f"msm-rows/{kind}")
    if kind == "zero":
        return [0] * N
    if kind == "one":
        return [1] * N
    if kind == "repeat":       # ONE dense value: each of its digits' buckets holds all N points — 4 125 partials of 8, the two-stage fold and its tickets
        return [rng.randrange(P >> 1, P)] * N
    if kind in ("random", "random2"):
        return [rng.randrange(P) for _ in range(N)]
    if kind == "neg_small":
        return [P - 1 - rng.getrandbits(139) for _ in range(N)]
    if kind == "ones40":
        return [1 if k < 0.4 else 0 if k < 0.6 else rng.randrange(P) for k in (rng.random() for _ in range(N))]
    if kind == "bytes":        # a witness's small values: bits, bytes, a few dense wires
        return [rng.randrange(2) if k < 0.5 else rng.randrange(256) if k < 0.9 else rng.randrange(P) for k in (rng.random() for _ in range(N))]
    raise ValueError(kind)


def main(out_path):
    from tests import _oracle
    from tests._oracle import from_limbs, to_limbs
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    orc = _oracle.load()
    ctx = hip.Context(0)
    lib = ctx.lib
    vp = C.c_void_p
    lib.vimz_test_msm_rows.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_int, vp, vp, vp]
    pts = lambda a: [[int(x) for x in from_limbs(a[8 * i:8 * i + 8])] for i in range(len(a) // 8)]      # noqa: E731
    res = {"groups": {}, "alone": {}}
    try:
        bases = orc.seq_bases(0, N)
        B = {0: ctx.bases_upload(0, bases), 1: ctx.bases_upload(0, bases).precompute(15)}
        rows = [to_limbs(row(k)) for k in KINDS]
        fill = random.Random("msm-rows/between")
        between = to_limbs([fill.randrange(P) for _ in range(STRIDE - N)])
        try:
            for tables in (0, 1):
                for i, k in enumerate(KINDS):
                    res["alone"][f"{tables}/{k}"] = pts(ctx.msm(B[tables], rows[i]))[0]
                for G, members in GROUPS.items():
                    sc = np.ascontiguousarray(np.concatenate([np.concatenate([rows[m], between]) for m in members]))
                    assert sc.shape == (G * STRIDE, 4)
                    out, s1, s1_ref = (np.full(8 * CALLS * G, 7, dtype=np.uint64), np.full(8 * CALLS * G, 7, dtype=np.uint64), np.full(8 * G, 7, dtype=np.uint64))
                    ctx._chk(lib.vimz_test_msm_rows(ctx.h, B[tables].h, hip._ptr(sc), N, STRIDE, G, _lib.FORM_CANONICAL, tables, N_ONES, CALLS,
                                                    hip._ptr(out), hip._ptr(s1), hip._ptr(s1_ref)))
                    res["groups"][f"{tables}/{G}"] = {"out": pts(out), "s1": pts(s1), "s1_ref": pts(s1_ref)}
            res["oracle"] = [int(x) for x in orc.msm(0, bases, rows[ORACLE_ROW], threads=8)]
            ones = [i for i, s in enumerate(row("ones40")[:N_ONES]) if s == 1]
            res["oracle_s1_ones40"] = [int(x) for x in orc.msm(0, bases[ones], to_limbs([1] * len(ones)), threads=8)]
        finally:
            for b in B.values():
                b.free()
    finally:
        ctx.close()
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print("msm rows probe ok", len(res["groups"]))


if __name__ == "__main__":
    main(sys.argv[1])
