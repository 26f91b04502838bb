"""GPU half of tests/test_gpu_spartan_kernels.py, a process of its own with VIMZ_HIP_LIBRARY=testing (`python -m tests._spartan_kernels_gpu OUT.json`): every
case of tests/_spartan_ref.py through the vimz_test_spartan_* hooks — the functions spartan_prove and ipa_prove run for each round.  Words leave as the hex of
their little-endian bytes; nothing is judged here.  The vectors of the k >= 19 cases are expanded from the case's seed on this side too: only messages, final
values and, for the 2^21 eq table, chunk digests and a few elements travel.  Test infrastructure."""
import ctypes as C
import json
import sys
import time

import numpy as np

from tests import _spartan_ref as S
from tests._oracle import CURVE_BASE, CURVE_SCALAR


def to_words(vals):
    """ints below 2^256 -> (n, 4) uint64, little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def big_words(kind, fid, k, which):
    """a k >= 19 vector as words, straight from the seed's bytes (31 an element)"""
    raw = np.frombuffer(S.big_vector_bytes(kind, fid, k, which), dtype=np.uint8).reshape(-1, 31)
    out = np.zeros((raw.shape[0], 32), dtype=np.uint8)
    out[:, :31] = raw
    return np.ascontiguousarray(out).view("<u8").astype(np.uint64)


def hex_of(arr):
    return np.ascontiguousarray(arr, dtype="<u8").tobytes().hex()


def ints_hex(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals).hex()


def point_words(pts):
    return to_words([c for P in pts for c in S.pt_words(P)]).reshape(-1, 8)


class Coo(C.Structure):
    _fields_ = [("row", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("nnz", C.c_size_t)]


def main(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    lib = ctx.lib
    vp, sz = C.c_void_p, C.c_size_t
    lib.vimz_test_spartan_eq.argtypes = [vp, C.c_int, vp, sz, vp]
    lib.vimz_test_spartan_sumcheck.argtypes = [vp, C.c_int, C.c_int, sz, vp, vp, vp, vp, vp]
    lib.vimz_test_spartan_ipa_vec.argtypes = [vp, C.c_int, sz, vp, vp, vp, vp, vp]
    lib.vimz_test_spartan_fold_bases.argtypes = [vp, C.c_int, vp, sz, vp, vp]
    lib.vimz_test_spartan_instance.argtypes = [vp, C.c_int, sz, sz, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_char_p, vp, sz]
    lib.vimz_test_spartan_instance.restype = C.c_int64
    lib.vimz_test_spartan_instance_verify.argtypes = [vp, C.c_int, sz, sz, vp, vp, vp, vp, vp, C.c_uint32, C.c_char_p, vp, C.c_int, vp, sz]
    ptr = hip._ptr

    def eq_raw(fid, pt_words, k):
        out = np.full((1 << min(k, 21), 4), 7, dtype=np.uint64)
        return lib.vimz_test_spartan_eq(ctx.h, fid, ptr(pt_words), k, ptr(out)), out

    def sumcheck_raw(fid, kind, k, vecs, u, chal):
        arr = (vp * 5)(*[v.ctypes.data if v is not None else None for v in vecs] + [None] * (5 - len(vecs)))
        per = 3 if kind == 0 else 2
        msgs, fin = np.full((per * k, 4), 7, dtype=np.uint64), np.full((5 if kind == 0 else 2, 4), 7, dtype=np.uint64)
        uw = to_words([u]) if u is not None else None
        rc = lib.vimz_test_spartan_sumcheck(ctx.h, fid, kind, k, C.cast(arr, vp), ptr(uw), ptr(chal), ptr(msgs), ptr(fin))
        return rc, msgs, fin

    def ipa_raw(fid, k, a, b, chal):
        dots, fin = np.full((2 * k, 4), 7, dtype=np.uint64), np.full((2, 4), 7, dtype=np.uint64)
        return lib.vimz_test_spartan_ipa_vec(ctx.h, fid, k, ptr(a), ptr(b), ptr(chal), ptr(dots), ptr(fin)), dots, fin

    def fold_raw(cid, pts_words, half, x):
        out = np.full((half, 8), 7, dtype=np.uint64)
        xw = np.array([x & (2 ** 64 - 1), x >> 64], dtype=np.uint64)
        return lib.vimz_test_spartan_fold_bases(ctx.h, cid, ptr(pts_words), half, ptr(xw), ptr(out)), out

    def chk(rc, *rest):
        ctx._chk(rc)
        return rest

    def rounds(msgs, fin):
        return {"msgs": hex_of(msgs), "finals": hex_of(fin)}

    res = {"eq": {}, "outer": {}, "inner": {}, "ipa": {}, "fold": {}, "instance": {}, "refused": {}}
    keys = {}
    try:
        # ---- the field side at k <= 10
        for fid in (0, 1):
            for k in S.SMALL_K:
                for name in S.small_case_names("eq"):
                    c = S.small_case("eq", fid, k, name)
                    res["eq"][f"{fid}/{k}/{name}"] = hex_of(chk(*eq_raw(fid, to_words(c["vecs"][0]), k))[0])
                for kind, code in (("outer", 0), ("inner", 1)):
                    for name in S.small_case_names(kind):
                        c = S.small_case(kind, fid, k, name)
                        vecs = [to_words(v) if v is not None else None for v in c["vecs"]]
                        res[kind][f"{fid}/{k}/{name}"] = rounds(*chk(*sumcheck_raw(fid, code, k, vecs, c["u"], to_words(c["chal"]))))
                for name in S.small_case_names("ipa"):
                    c = S.small_case("ipa", fid, k, name)
                    res["ipa"][f"{fid}/{k}/{name}"] = rounds(*chk(*ipa_raw(fid, k, to_words(c["vecs"][0]), to_words(c["vecs"][1]), to_words(c["chal"]))))
        # ---- the striding cases
        fid, k = S.OUTER_BIG
        u, chal = S.big_scalars("outer", fid, k)
        vecs = [big_words("outer", fid, k, w) for w in range(5)]
        res["outer"][f"{fid}/{k}/big"] = rounds(*chk(*sumcheck_raw(fid, 0, k, vecs, u, to_words(chal))))
        fid, k = S.IPA_BIG
        _, chal = S.big_scalars("ipa", fid, k)
        res["ipa"][f"{fid}/{k}/big"] = rounds(*chk(*ipa_raw(fid, k, big_words("ipa", fid, k, 0), big_words("ipa", fid, k, 1), to_words(chal))))
        fid, k = S.INNER_BIG
        _, chal = S.big_scalars("inner", fid, k)
        vecs = [big_words("inner", fid, k, w) for w in range(2)]
        res["inner"][f"{fid}/{k}/big"] = rounds(*chk(*sumcheck_raw(fid, 1, k, vecs, None, to_words(chal))))
        del vecs
        fid, k = S.EQ_BIG
        _, chal = S.big_scalars("eq", fid, k)
        tab, = chk(*eq_raw(fid, to_words(chal), k))
        raw = np.ascontiguousarray(tab, dtype="<u8").tobytes()
        res["eq"][f"{fid}/{k}/big"] = {"digests": S.table_digests(raw), "samples": {str(i): raw[32 * i:32 * i + 32].hex() for i in S.EQ_SAMPLES(1 << k)}}
        del tab, raw
        # ---- the generator folding
        for cid in (0, 1):
            for name in S.fold_case_names():
                pts, x = S.fold_case(cid, name)
                res["fold"][f"{cid}/{name}"] = hex_of(chk(*fold_raw(cid, point_words(pts), len(pts) // 2, x))[0])
        # ---- whole instances
        for cid in (0, 1):
            keys[cid] = ctx.bases_upload(cid, point_words(S.key_points(cid)))

        def coos(case, drop=None):
            keep, out = [], []
            for m in "ABC":
                trip = case[m]
                r, c = np.array([t[0] for t in trip], dtype=np.uint32), np.array([t[1] for t in trip], dtype=np.uint32)
                v = to_words([t[2] for t in trip])
                keep += [r, c, v]
                out.append(Coo(r.ctypes.data, c.ctypes.data, v.ctypes.data, len(trip)))
            return keep, out

        def prove(case, key=None, n_c=None, n_w=None, cid=None, Z=None, digest=None):
            cid = case["cid"] if cid is None else cid
            keep, (A, B, Cm) = coos(case)
            Zw = to_words(case["Z"] if Z is None else Z)
            Ew = to_words(case["E"]) if case["E"] is not None else None
            cap = 128 + S.argument_size(case)
            buf = np.full(cap // 8, 7, dtype=np.uint64)
            n = lib.vimz_test_spartan_instance(ctx.h, cid, case["n_c"] if n_c is None else n_c, case["n_w"] if n_w is None else n_w, C.byref(A), C.byref(B), C.byref(Cm),
                                               ptr(Zw), ptr(Ew), (keys[case["cid"]] if key is None else key).h, ptr(to_words([case["digest"] if digest is None else digest])),
                                               case["side_tag"], S.LABEL, ptr(buf), cap)
            return n, buf

        def verify(case, blob, X0_delta=0):
            keep, (A, B, Cm) = coos(case)
            ps = S.FIELD[CURVE_SCALAR[case["cid"]]]
            inst = np.concatenate([np.frombuffer(blob[:128], dtype="<u8").astype(np.uint64),
                                   to_words([case["Z"][0], (case["Z"][case["n_w"] - 2] + X0_delta) % ps, case["Z"][case["n_w"] - 1]]).reshape(-1)])
            words = np.frombuffer(blob[128:], dtype="<u8").astype(np.uint64)
            return lib.vimz_test_spartan_instance_verify(ctx.h, case["cid"], case["n_c"], case["n_w"], C.byref(A), C.byref(B), C.byref(Cm), keys[case["cid"]].h,
                                                         ptr(to_words([case["digest"]])), case["side_tag"], S.LABEL, ptr(inst), int(case["E"] is not None), ptr(words), words.size)

        for name in S.instance_names():
            case = S.instance_case(name)
            n, buf = prove(case)
            if n != 128 + S.argument_size(case):
                ctx._chk(int(n) if n < 0 else 0)
                raise AssertionError(f"{name}: {n} bytes, expected {128 + S.argument_size(case)}")
            blob = buf.tobytes()
            res["instance"][name] = {"blob": blob.hex(), "verify": verify(case, blob), "x0_plus_1": verify(case, blob, X0_delta=1),
                                     "tamper": {what: verify(case, S.flip(blob, 128 + off)) for what, off in S.argument_layout(case).items()}}
        again = S.instance_names()[5]
        res["repeat"] = {"name": again, "blobs": [prove(S.instance_case(again))[1].tobytes().hex() for _ in range(2)]}
        # ---- what the hooks refuse
        ref = res["refused"]
        one = to_words([1, 2])
        pR, pQ = S.FIELD[0], S.FIELD[1]
        ref["eq_field"] = eq_raw(2, one, 1)[0]
        ref["eq_k_0"] = eq_raw(0, one, 0)[0]
        ref["eq_k_22"] = eq_raw(0, to_words([1] * 22), 22)[0]
        ref["eq_not_reduced"] = eq_raw(0, to_words([pR]), 1)[0]
        ref["eq_not_reduced_fq"] = eq_raw(1, to_words([pQ]), 1)[0]
        v2 = [to_words([1, 2])] * 5
        ref["sumcheck_field"] = sumcheck_raw(3, 0, 1, v2, 1, to_words([5]))[0]
        ref["sumcheck_vector_not_reduced"] = sumcheck_raw(0, 0, 1, v2[:2] + [to_words([1, pR])] + v2[3:], 1, to_words([5]))[0]
        ref["sumcheck_u_not_reduced"] = sumcheck_raw(0, 0, 1, v2, pR, to_words([5]))[0]
        ref["sumcheck_challenge_not_reduced"] = sumcheck_raw(0, 1, 1, v2[:2], None, to_words([pR]))[0]
        ref["ipa_field"] = ipa_raw(2, 1, one, one, to_words([5]))[0]
        ref["ipa_not_reduced"] = ipa_raw(0, 1, to_words([pR + 1, 0]), one, to_words([5]))[0]
        g = S.fold_pool(0)[:2]
        ref["fold_curve"] = fold_raw(2, point_words(g), 1, 5)[0]
        ref["fold_half_0"] = fold_raw(0, point_words(g), 0, 5)[0]
        ref["fold_coordinate_not_reduced"] = fold_raw(0, point_words([g[0], (g[1][0] + S.CURVES[0][0], g[1][1])]), 1, 5)[0]
        small = S.instance_case(S.instance_names()[0])              # 4 x 2
        ref["instance_curve"] = prove(small, cid=2)[0]
        ref["instance_n_w_3"] = prove(small, n_w=3)[0]
        ref["instance_n_c_1"] = prove(small, n_c=1)[0]
        ref["instance_z_not_reduced"] = prove(small, Z=[pR] + small["Z"][1:])[0]
        ref["instance_digest_not_reduced"] = prove(small, digest=pR)[0]
        wide = S.instance_case("0/300x17/strict")
        short = ctx.bases_upload(0, point_words(S.key_points(0)[:511]))
        ref["instance_key_shorter_than_padded_shape"] = prove(wide, key=short)[0]
        short.free()
        ref["instance_key_of_the_other_curve"] = prove(small, key=keys[1])[0]
        n, buf = prove(small)
        res["accepted_after"] = {"rc": int(n), "same": buf.tobytes().hex() == res["instance"][S.instance_names()[0]]["blob"],
                                 "eq": eq_raw(0, to_words(S.small_case("eq", 0, 3, "random")["vecs"][0]), 3)[1].tobytes().hex() == res["eq"]["0/3/random"]}
        res["refused"] = {k: int(v) for k, v in ref.items()}
    finally:
        for kb in keys.values():
            kb.free()
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"spartan kernels probe ok: {len(res['eq'])} tables, {len(res['outer'])} + {len(res['inner'])} sum-checks, {len(res['ipa'])} vector foldings, "
          f"{len(res['fold'])} base foldings, {len(res['instance'])} instances, {res['seconds']:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1])
