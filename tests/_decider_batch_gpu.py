"""GPU half of tests/test_gpu_decider_batch.py, a process of its own per part with VIMZ_HIP_LIBRARY=testing (`python -m tests._decider_batch_gpu {kernels|decider}
OUT.json`): the batched decider verifier (vimz_decider_verify_batch; vimz_amd/csrc/decider_batch.hip).

kernels: k_miller through vimz_test_miller_loops and k_g1_lincomb through vimz_test_g1_lincomb at n = 1, 2, 63, 64, 65 over the first n of miller_pairs() and
lincomb_rows().
decider: once, on the light decider of the hash step: three proofs of one prover at 2, 3 and 4 steps, batches of them and of tampered copies through the device path,
the host path, Decider.verify_batch and Decider.verify, and two proofs with their C points swapped with multipliers that are all one and with the OS's.
Words leave as integers and nothing is judged here.  Test infrastructure."""
import ctypes as C
import json
import sys
import time

import numpy as np

from tests import _miller_ref as M
from tests import _pairing as bp

SIZES = (1, 2, 63, 64, 65)
Q, R = bp.Q, bp.R


def miller_pairs():
    """65 pairs (P or None, Q or None): the generators, P the identity, Q the identity, P and −P against one Q, then multiples that walk from random starts"""
    p, q = bp.g1_mul(bp.G1, 0x1F2E3D4C5B6A79881726354), bp.g2_mul(bp.G2, 0xABCDEF0123456789ABCDEF0123)
    pairs = [(bp.G1, bp.G2), (None, q), (p, None), (p, q), (bp.g1_neg(p), q)]
    dp, dq = bp.g1_mul(bp.G1, 0x9E3779B97F4A7C15), bp.g2_mul(bp.G2, 0xC2B2AE3D27D4EB4F)
    while len(pairs) < 65:
        p, q = bp.g1_add(p, dp), bp.g2_add(q, dq)
        pairs.append((p, q))
    return pairs


def lincomb_rows():
    """65 rows (a, k, bits, b): a the identity, b the identity, k = 0, k = r − 1 with a = b, then walks of 1, 128 and 254 bits in turn"""
    rows = []
    a, b = bp.g1_mul(bp.G1, 1000), bp.g1_mul(bp.G1, 2000)
    for i in range(65):
        k = (0x2FFFFFFFFFFFFFFF << 192) | ((0x165667B19E3779F9 + i) << 128) | ((0xC2B2AE3D27D4EB4F ^ i) << 64) | (0x9E3779B97F4A7C15 * (i + 1) % (1 << 64))
        row = [a, k, (1, 128, 254)[i % 3], b]
        if i == 0:
            row[0] = None
        elif i == 1:
            row[3] = None
        elif i == 2:
            row[1] = 0
        elif i == 3:
            row = [b, R - 1, 254, b]
        rows.append(tuple(row))
        a, b = bp.g1_add(a, bp.G1), bp.g1_add(b, bp.g1_mul(bp.G1, 3))
    return rows


def lincomb_expected(row):
    a, k, bits, b = row
    return bp.g1_add(a, None if b is None else bp.g1_mul(b, k & ((1 << bits) - 1)))


def words64(values, per):
    """integers -> uint64 rows of `per` words"""
    return np.frombuffer(b"".join(int(v).to_bytes(8 * per, "little") for v in values), dtype="<u8").astype(np.uint64).reshape(len(values), per)


def g1_words(p):
    return [0, 0] if p is None else [p[0], p[1]]


def g2_words(q):
    return [0, 0, 0, 0] if q is None else [q[0][0], q[0][1], q[1][0], q[1][1]]


def open_context():
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    vp, st = C.c_void_p, C.c_size_t
    ctx.lib.vimz_test_miller_loops.argtypes = [vp, vp, vp, st, vp]
    ctx.lib.vimz_test_g1_lincomb.argtypes = [vp, vp, vp, vp, vp, st, vp]
    return ctx


def main_kernels(out_path):
    t_start = time.time()
    from vimz_amd import hip
    ctx = open_context()
    res = {"miller": {}, "lincomb": {}}
    try:
        pairs, rows = miller_pairs(), lincomb_rows()
        for n in SIZES:
            g1 = words64([c for p, _ in pairs[:n] for c in g1_words(p)], 4)
            g2 = words64([c for _, q in pairs[:n] for c in g2_words(q)], 4)
            out = np.full(96 * n, 7, dtype=np.uint32)
            ctx._chk(ctx.lib.vimz_test_miller_loops(ctx.h, hip._ptr(g1), hip._ptr(g2), n, hip._ptr(out)))
            res["miller"][str(n)] = [int(x) for x in out]
            a = words64([c for r in rows[:n] for c in g1_words(r[0])], 4)
            b = words64([c for r in rows[:n] for c in g1_words(r[3])], 4)
            k = words64([r[1] for r in rows[:n]], 4)
            bits = np.array([r[2] for r in rows[:n]], dtype=np.uint32)
            o = np.full((2 * n, 4), 7, dtype=np.uint64)
            ctx._chk(ctx.lib.vimz_test_g1_lincomb(ctx.h, hip._ptr(a), hip._ptr(k), hip._ptr(bits), hip._ptr(b), n, hip._ptr(o)))
            res["lincomb"][str(n)] = [str(sum(int(o[i, q]) << (64 * q) for q in range(4))) for i in range(2 * n)]
        off = words64([1, 3], 4)
        res["bad_arguments"] = {"n_0": ctx.lib.vimz_test_miller_loops(ctx.h, hip._ptr(g1), hip._ptr(g2), 0, hip._ptr(out)),
                                "off_curve": ctx.lib.vimz_test_g1_lincomb(ctx.h, hip._ptr(off), hip._ptr(k), hip._ptr(bits), hip._ptr(off), 1, hip._ptr(o)),
                                "bits_257": ctx.lib.vimz_test_g1_lincomb(ctx.h, hip._ptr(a), hip._ptr(k), hip._ptr(np.array([257], dtype=np.uint32)), hip._ptr(b), 1, hip._ptr(o))}
    finally:
        ctx.close()
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"decider batch kernels probe ok: sizes {SIZES}, {res['seconds']:.1f} s")


def main_decider(out_path):
    t_start = time.time()
    from tests.test_circuits import step_inputs
    from vimz_amd import _lib, calldata, hip
    from vimz_amd.circuit import Circuit
    ctx = open_context()
    res = {}
    c = Circuit.for_resolution("hash", "HD")
    srs, kzg_vk = hip.kzg_setup(ctx, 36000)
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
    cf = hip.CycleFoldIVC(ctx, c, srs, ck2, max_batch=2)
    dec = None
    try:
        z0, inputs = step_inputs("hash")
        proofs = []
        for steps in (2, 3, 4):
            cf.reset(z0); cf.fold(np.stack(inputs[:steps]))
            if dec is None:
                dec = hip.Decider(cf, kzg_vk=kzg_vk, light=True)
            _, d = calldata.decider_calldata(dec)
            assert d["steps"] == steps
            proofs.append((d["steps"], d["z0"], d["z_i"], d["words"]))
        kw = dec.key_words()
        res["single"] = [dec.verify(*p) for p in proofs]
        res["three"] = {str(chunk): dec.verify_batch(proofs, chunk=chunk) for chunk in (0, 1, 2)}

        def changed(p, at, fn):
            w = list(p[3]); w[at] = fn(w[at])
            return (p[0], p[1], p[2], w)
        seven = [proofs[0], changed(proofs[0], 22, lambda v: Q - v), changed(proofs[1], 24, lambda v: Q - v), proofs[1], changed(proofs[2], 16, lambda v: Q - v), proofs[2],
                 changed(proofs[0], 0, lambda v: v ^ 1)]
        sec = {}
        res["seven"] = {"single": [dec.verify(*p) for p in seven], "key": [hip.decider_verify_key(kw, *p) for p in seven],
                        "device": {str(chunk): hip.verify_decider_batch(ctx, kw, seven, chunk=chunk, seconds=sec) for chunk in (2, 0)},
                        "host": hip.verify_decider_batch(None, kw, seven, chunk=2), "seconds": sec}
        res["empty"] = hip.verify_decider_batch(ctx, kw, [])
        # two valid proofs with their C points swapped
        a, b = proofs[0], proofs[1]
        wa, wb = list(a[3]), list(b[3])
        wa[15:17], wb[15:17] = b[3][15:17], a[3][15:17]
        swapped = [(a[0], a[1], a[2], wa), (b[0], b[1], b[2], wb)]
        res["swapped"] = {"single": [dec.verify(*p) for p in swapped], "ones": hip.verify_decider_batch(ctx, kw, swapped, multipliers=[1] * 6),
                          "ones_host": hip.verify_decider_batch(None, kw, swapped, multipliers=[1] * 6), "production": hip.verify_decider_batch(ctx, kw, swapped),
                          "restated_ones": bool(M.batch_accepts(dec.verifying_key(), swapped, [(1, 1, 1)] * 2))}
        try:
            hip.verify_decider_batch(ctx, kw[:-1], proofs)
            res["bad_key"] = "accepted"
        except _lib.VimzError as e:
            res["bad_key"] = str(e)
    finally:
        if dec is not None:
            dec.close()
        cf.close(); srs.free(); ck2.free(); ctx.close()
    res["seconds_total"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"decider batch probe ok: {res['seconds_total']:.1f} s; the batch of seven on the device: {res['seven']['seconds']}")


if __name__ == "__main__":
    {"kernels": main_kernels, "decider": main_decider}[sys.argv[1]](sys.argv[2])
