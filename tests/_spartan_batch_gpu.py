"""GPU half of tests/test_gpu_spartan_batch.py, a process a part with VIMZ_HIP_LIBRARY=testing (`python -m tests._spartan_batch_gpu PART OUT.json`): the cases of
tests/_spartan_batch_ref.py through the hooks of the batched compressed-proof verifier (vimz_amd/csrc/spartan_batch.hpp), and the two entry points end to end on
`hash` at HD.  Nothing is judged here but what needs the device's own answer (a batch against the single entry, member by member).  Test infrastructure.
Parts: svec, mat, instance, ivc, cf."""
import ctypes as C
import json
import sys
import time

import numpy as np

from tests import _spartan_batch_ref as B
from tests import _spartan_pub_ref as P
from tests import _spartan_ref as S
from tests._oracle import CURVE_SCALAR
from tests._spartan_kernels_gpu import Coo, point_words, to_words

vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32


def _setup(lib):
    lib.vimz_test_spartan_mat_eval.argtypes = [vp, C.c_int, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.vimz_test_spartan_svec_accum.argtypes = [vp, C.c_int, u32, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.vimz_test_spartan_instance_batch.argtypes = [vp, C.c_int, sz, sz, u32, vp, vp, vp, vp, vp, u32, C.c_char_p, sz, vp, vp, vp, vp, sz, vp, vp, C.POINTER(C.c_double), vp]
    lib.vimz_test_spartan_instance_pub_verify.argtypes = [vp, C.c_int, sz, sz, u32, vp, vp, vp, vp, vp, u32, C.c_char_p, vp, C.c_int, vp, sz]


def coos(c):
    keep, out = [], []
    for m in "ABC":
        trip = c[m]
        r, col = np.array([t[0] for t in trip], dtype=np.uint32), np.array([t[1] for t in trip], dtype=np.uint32)
        v = to_words([t[2] for t in trip]) if trip else np.zeros((1, 4), dtype=np.uint64)
        keep += [r, col, v]
        out.append(Coo(r.ctypes.data if trip else None, col.ctypes.data if trip else None, v.ctypes.data if trip else None, len(trip)))
    return keep, out


def ints_of(arr):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(arr, dtype="<u8").reshape(-1, 4)]


def svec_run(ctx, case):
    from vimz_amd import hip
    ptr = hip._ptr
    ops, rounds = case["ops"], case["rounds"]
    xs = to_words([x for op in ops for x in op["xs"]])
    pts = to_words([x for op in ops for x in op["pt"]])
    cf = to_words([op["coef"] for op in ops])
    sh = np.array([int(op["shifted"]) for op in ops], dtype=np.uint32)
    npub = np.array([op["n_pub"] for op in ops], dtype=np.uint32)
    nw = np.array([op["n_w"] for op in ops], dtype=np.uint32)
    acc = np.full((1 << rounds, 4), 7, dtype=np.uint64)
    dots = np.full((len(ops), 4), 7, dtype=np.uint64)
    ctx._chk(ctx.lib.vimz_test_spartan_svec_accum(ctx.h, case["fid"], rounds, len(ops), ptr(xs), ptr(pts), ptr(cf), ptr(sh), ptr(npub), ptr(nw), ptr(acc), ptr(dots)))
    return acc, dots


def part_svec(ctx, res):
    res["group"], res["split"] = int(ctx.lib.vimz_test_spartan_batch_group()), int(ctx.lib.vimz_test_spartan_batch_split())
    res["case"] = {}
    for name in B.svec_case_names():
        acc, dots = svec_run(ctx, B.svec_case(name))
        res["case"][name] = {"acc": acc.tobytes().hex(), "dots": [str(v) for v in ints_of(dots)]}
    acc, dots = svec_run(ctx, B.svec_big_case())
    res["big"] = {"digests": S.table_digests(np.ascontiguousarray(acc, dtype="<u8").tobytes()), "dots": [str(v) for v in ints_of(dots)]}


def mat_run(ctx, case, members):
    from vimz_amd import hip
    ptr = hip._ptr
    keep, (A, Bm, Cm) = coos(case)
    rx = to_words([x for m in members for x in m[0]])
    ry = to_words([x for m in members for x in m[1]])
    w = to_words([x for m in members for x in m[2]])
    out = np.full((len(members), 4), 7, dtype=np.uint64)
    ctx._chk(ctx.lib.vimz_test_spartan_mat_eval(ctx.h, case["cid"], case["n_c"], case["n_w"], C.byref(A), C.byref(Bm), C.byref(Cm), len(members), ptr(rx), ptr(ry), ptr(w),
                                                ptr(out)))
    return [str(v) for v in ints_of(out)]


def part_mat(ctx, res):
    res["shape"], res["special"] = {}, {}
    for name in B.mat_shape_cases():
        case = S.instance_case(name)
        res["shape"][name] = {str(n): mat_run(ctx, case, B.mat_points(case, n, name)) for n in B.MAT_GROUPS}
    for cid in (0, 1):
        for kind in ("mixed", "empty"):
            case = B.mat_special_case(cid, kind)
            key = f"{cid}/{kind}"
            res["special"][key] = {str(n): mat_run(ctx, case, B.mat_points(case, n, key)) for n in B.MAT_GROUPS}


INSTANCE_SHAPES = {0: "0/5x12x2", 1: "1/3x17x7"}          # (n_c x n_w x n_pub of tests/_spartan_pub_ref.py)


def part_instance(ctx, res, orc):
    """per curve: the relaxed and the strict instance of one shape, proved by the integer prover; members of a batch are copies of the two, honest or tampered"""
    from vimz_amd import _lib, hip
    ptr = hip._ptr
    lib = ctx.lib
    for cid, shape in INSTANCE_SHAPES.items():
        key = ctx.bases_upload(cid, point_words(S.key_points(cid)))
        try:
            # ONE shape for every member: the strict case's matrices (its C rows make Az∘Bz = Cz hold for its own Z at u = 1); any other Z satisfies the RELAXED
            # relation over them with E = Az∘Bz − u·Cz
            strict = P.case(shape + "/strict")
            ps = S.FIELD[CURVE_SCALAR[cid]]
            rng = S._rng("batch-instance", cid)
            c = dict(strict)
            c["Z"] = [rng.randrange(1, ps) for _ in range(strict["n_w"])]
            az, bz, cz = S.products(c)
            c["E"] = [(x * y - c["Z"][0] * w) % ps for x, y, w in zip(az, bz, cz)]
            _, blob = P.prove(orc, c)
            keep, (A, Bm, Cm) = coos(c)
            dg = to_words([c["digest"]])
            stride = 16 + 4 * (1 + c["n_pub"])
            u, X = c["Z"][0], list(c["Z"][c["n_w"] - c["n_pub"]:])

            def single(b, uu, XX, has_E=1, tag=None):
                inst = np.concatenate([np.frombuffer(b[:128], dtype="<u8").astype(np.uint64), to_words([uu] + list(XX)).reshape(-1)])
                words = np.frombuffer(b[128:], dtype="<u8").astype(np.uint64)
                return int(lib.vimz_test_spartan_instance_pub_verify(ctx.h, cid, c["n_c"], c["n_w"], len(XX), C.byref(A), C.byref(Bm), C.byref(Cm), key.h, ptr(dg),
                                                                     c["side_tag"] if tag is None else tag, P.LABEL, ptr(inst), has_E, ptr(words), words.size))

            def batch(members, chunk, mult=None, want_acc=False, raw_rc=False):
                """members: [(blob, u, X, has_E)]"""
                n = len(members)
                inst = np.zeros((max(n, 1), stride), dtype=np.uint64)
                arrs = []
                for i, (b, uu, XX, hE) in enumerate(members):
                    inst[i, :16] = np.frombuffer(b[:128], dtype="<u8")
                    inst[i, 16:] = to_words([uu] + list(XX)).reshape(-1)
                    arrs.append(np.frombuffer(b[128:], dtype="<u8").astype(np.uint64))
                wp = (vp * max(n, 1))(*[a.ctypes.data for a in arrs])
                wn = (sz * max(n, 1))(*[a.size for a in arrs])
                hE = np.array([m[3] for m in members] + [0], dtype=np.int32)
                out = np.full(max(n, 1), 7, dtype=np.uint32)
                sec = (C.c_double * 6)()
                big = 1 << (max(c["n_c"], c["n_w"]) - 1).bit_length()
                acc = np.zeros((big, 4), dtype=np.uint64) if want_acc else None
                m = np.ascontiguousarray(to_words(mult)[:, :2]) if mult is not None else None
                rc = lib.vimz_test_spartan_instance_batch(ctx.h, cid, c["n_c"], c["n_w"], c["n_pub"], C.byref(A), C.byref(Bm), C.byref(Cm), key.h, ptr(dg), c["side_tag"],
                                                          P.LABEL, n, ptr(inst), ptr(hE), C.cast(wp, vp), C.cast(wn, vp), chunk, ptr(m), ptr(out), sec, ptr(acc))
                if raw_rc:
                    return rc
                ctx._chk(rc)
                return {"results": [int(x) for x in out[:n]], "seconds": list(sec), "acc": [str(v) for v in ints_of(acc)] if want_acc else None}

            good = (blob, u, X, 1)
            bumpW, bumpE = B.bump_final_scalar(c, blob, "W"), B.bump_final_scalar(c, blob, "E")
            out = {"single_good": single(blob, u, X), "single_bumpW": single(bumpW, u, X), "single_bumpE": single(bumpE, u, X)}
            out["honest"] = {str(ch): batch([good] * 5, ch)["results"] for ch in (0, 1, 2)}
            out["empty"] = batch([], 0)["results"]
            mixed = [good, (bumpW, u, X, 1), good, good, (bumpE, u, X, 1)]
            out["mixed"] = {str(ch): batch(mixed, ch) for ch in (0, 1, 2)}
            # X_k + 1 and u + 1: the single hook's verdict, member by member
            pub = [good, (blob, (u + 1) % ps, X, 1)] + [(blob, u, X[:k] + [(X[k] + 1) % ps] + X[k + 1:], 1) for k in range(len(X))]
            out["public"] = {"single": [single(m[0], m[1], m[2]) for m in pub], "batch": {str(ch): batch(pub, ch)["results"] for ch in (0, 2)}}
            # a strict instance (no E opening, cl[3] = 0) beside relaxed ones, honest and with its final scalar + 1
            _, sblob = P.prove(orc, strict)
            su, sX = strict["Z"][0], list(strict["Z"][strict["n_w"] - strict["n_pub"]:])
            smem = [good, (sblob, su, sX, 0), good, (B.bump_final_scalar(strict, sblob, "W"), su, sX, 0), (blob, u, X, 0)]
            out["strict_beside"] = {"single": [single(m[0], m[1], m[2], m[3]) for m in smem], "batch": {str(ch): batch(smem, ch)["results"] for ch in (0, 2)}}
            # multipliers: all one -> the accumulators of the reference; a zero one is refused
            ones = batch([good, good, good], 0, mult=[1] * 6, want_acc=True)
            out["ones"] = ones
            out["zero_multiplier"] = batch([good, good], 0, mult=[1, 1, 0, 1], raw_rc=True)
            out["production_bump"] = [batch([good, (bumpW, u, X, 1)], 0)["results"] for _ in range(3)]
            res[str(cid)] = out
        finally:
            key.free()
    res["invalid"] = _lib.ERR_INVALID


def _arg_words(s, t, e):
    return 4 * (3 * s + 4 + 2 * t + 1) + 4 * (4 * t + 1) + (4 * (4 * s + 1) if e else 0)


def part_family(ctx, res, family):
    """`hash` at HD: two one-chain and two merged proofs of different step counts, tampered copies, a truncated blob, a blob of the other family; the batch's
    words against the single entries' at chunk 0, 1 and 2, and through folding.verify_compressed_proofs"""
    from tests.test_circuits import step_inputs
    from vimz_amd import folding
    mode = "cyclefold" if family == "cf" else "ivc"
    other_mode = "ivc" if family == "cf" else "cyclefold"
    circuit, params = folding.prepare_folding(ctx, "hash", "HD", backend="sonobe")
    z0, inputs = step_inputs("hash")
    rows = np.stack(inputs)
    proofs, made = [], []
    try:
        def make(md, n_rows, segments):
            pr = folding.fold_input(params, rows[:n_rows], z0, max_batch=4, mode=md, segments=segments)
            made.append(pr)
            blob, _ = folding.compress_proof(params, pr)
            return pr, np.array(blob, dtype=np.uint8)

        pr_chain, chain5 = make(mode, 5, 1)
        _, chain3 = make(mode, 3, 1)
        _, merged6 = make(mode, 6, 2)
        _, merged4 = make(mode, 4, 2)
        _, other = make(other_mode, 3, 1)
        vk = pr_chain.prover
        hdr = np.frombuffer(chain5[:64].tobytes(), dtype="<u8")
        s1, t1, s2, t2 = (int(x) for x in hdr[3:7])
        if family == "ivc":
            tail = [_arg_words(s2, t2, True), _arg_words(s2, t2, False)]          # primary | secondary | fresh
        else:
            tail = [_arg_words(s1, t1, False), _arg_words(s2, t2, True)]          # running | fresh | cyclefold
        members = []          # (what, blob, steps, z0)

        def flipped(b, off):
            out = b.copy(); out[off] ^= 1
            return out

        zbad = [int(z0[0]) + 1] + [int(z) for z in z0[1:]]
        members += [("chain5", chain5, 5, z0), ("chain5 steps+1", chain5, 6, z0), ("merged6", merged6, 6, z0), ("chain5 other z0", chain5, 5, zbad),
                    ("chain3", chain3, 3, z0), ("chain5 last argument", flipped(chain5, len(chain5) - 32), 5, z0),
                    ("merged4", merged4, 4, z0), ("chain5 middle argument", flipped(chain5, len(chain5) - 8 * tail[1] - 32), 5, z0),
                    ("chain3 first argument", flipped(chain3, len(chain3) - 8 * (tail[0] + tail[1]) - 32), 3, z0),
                    ("merged6 last argument", flipped(merged6, len(merged6) - 32), 6, z0),
                    ("chain5 instance", flipped(chain5, 8 * (8 + 8 * circuit.len_z) + 8), 5, z0),
                    ("merged6 first argument", flipped(merged6, len(merged6) - 8 * _arg_words(s2, t2, True) - 32), 6, z0),
                    ("merged4 steps-1", merged4, 3, z0), ("chain5 sum-check message", flipped(chain5, len(chain5) - 8 * (tail[0] + tail[1]) - 8 * _arg_words(s1, t1, True) + 8), 5, z0),
                    ("chain3 truncated", chain3[:-8], 3, z0), ("other family", other, 3, z0), ("merged6 truncated", merged6[:-16], 6, z0)]
        # the SECOND hash (bit 1) with the blob left well-formed: an element that is read without a curve check and enters that hash alone.  Nova: U1.X0 (a 256-bit
        # integer) of the chain's instances and of the first segment's record; Nova + CycleFold: cfU.u of the same two places.
        lz = circuit.len_z
        inst = 8 + 8 * lz
        if family == "ivc":
            seg0 = 2 + 8
            at_chain, at_merged = inst + 20, seg0 + 1 + 8 * lz + 20
        else:
            runs = int(np.frombuffer(merged6[8 * (2 + 7):8 * (2 + 8)].tobytes(), dtype="<u8")[0])
            seg0 = 2 + 8 + runs
            at_chain, at_merged = inst + 60, seg0 + 1 + 8 * lz + 60
        members += [("chain5 second hash", flipped(chain5, 8 * at_chain), 5, z0), ("merged6 second hash", flipped(merged6, 8 * at_merged), 6, z0)]
        single = []
        t0 = time.time()
        for what, b, n, z in members:
            try:
                folding.verify_compressed_proof(vk, b, n, z)
                single.append(0)
            except Exception as e:          # noqa: BLE001  (the word is in the message; a blob of the other family is refused before the library sees it)
                msg = str(e)
                single.append(int(msg.split("flags ")[1].rstrip(")"), 16) if "flags " in msg else 8192)
        t_single = time.time() - t0
        blobs, steps, zs = [m[1] for m in members], [m[2] for m in members], [m[3] for m in members]
        out = {"what": [m[0] for m in members], "single": single, "single_s": t_single, "batch": {}, "seconds": {}}
        for ch in (0, 1, 2):
            t0 = time.time()
            words, sec = vk.verify_compressed_batch(blobs, steps, zs, chunk=ch)
            out["batch"][str(ch)] = words
            out["seconds"][str(ch)] = dict(sec, wall_s=time.time() - t0)
        out["folding"] = folding.verify_compressed_proofs(vk, [b.tobytes() for b in blobs], steps, zs)
        out["empty"] = folding.verify_compressed_proofs(vk, [], [], [])
        honest = [m for m in members if m[0] in ("chain5", "merged6", "chain3", "merged4")]
        words, sec = vk.verify_compressed_batch([m[1] for m in honest], [m[2] for m in honest], [m[3] for m in honest])
        out["honest"] = {"words": words, "seconds": sec}
        # the entry with GIVEN multipliers (six a proof): all one gives the single verifier's words; a zero one is refused.  A z0 element not below the modulus is
        # refused for the whole call, on the calling thread, whichever members carry it
        from vimz_amd import _lib, hip
        twin = f"vimz_testing_{family}_verify_compressed_batch_scalars"
        ones = np.zeros((6 * len(blobs), 2), dtype=np.uint64); ones[:, 0] = 1
        out["ones"] = {str(ch): hip._compressed_batch(vk, twin, blobs, steps, zs, ch, multipliers=ones)[0] for ch in (0, 2)}
        zero = ones.copy(); zero[6 * 2 + 1] = 0          # (the third proof's second multiplier)
        codes = {}
        for name, call in (("zero_multiplier", lambda: hip._compressed_batch(vk, twin, blobs, steps, zs, 0, multipliers=zero)),
                           ("bad_z0", lambda: vk.verify_compressed_batch(blobs[:4], steps[:4], [zs[0], [(1 << 256) - 1] + list(zs[1][1:]), zs[2], [(1 << 256) - 1] + list(zs[3][1:])]))):
            try:
                call()
                codes[name] = 0
            except _lib.VimzError as e:
                codes[name] = e.code
        out["codes"], out["invalid"] = codes, _lib.ERR_INVALID
        res[family] = out
    finally:
        for pr in made:
            pr.close()
        params.free()


def main(part, out_path):
    t_start = time.time()
    from tests import _oracle
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    _setup(ctx.lib)
    res = {}
    try:
        if part == "svec":
            part_svec(ctx, res)
        elif part == "mat":
            part_mat(ctx, res)
        elif part == "instance":
            part_instance(ctx, res, _oracle.load())
        elif part in ("ivc", "cf"):
            part_family(ctx, res, part)
        else:
            raise SystemExit(f"unknown part {part!r}")
    finally:
        ctx.close()
    res["seconds_total"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"spartan batch probe, part {part}: ok, {res['seconds_total']:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
