"""The cases of the batch verifiers' bisection (vimz_amd/csrc/batch_bisect.hpp) and the GPU half of tests/test_gpu_decider_batch_bisect.py and
tests/test_gpu_spartan_batch_bisect.py, a process a part with VIMZ_HIP_LIBRARY=testing (`python -m tests._batch_bisect_gpu PART OUT.json`).  Nothing is judged
here: the words and the counts go out as they come.  Test infrastructure.  Parts: decider, instance, cf."""
import ctypes as C
import json
import sys
import time

import numpy as np

from tests import _batch_bisect_ref as R

vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32

CHUNKS = (7, 4, 2)
LEAVES = (1, 2)


def patterns(n):
    """the bad sets of a batch of n: the first member, the last, a pair in the middle, both ends, every member"""
    return {"first": (0,), "last": (n - 1,), "pair": (2, 3), "ends": (0, n - 1), "all": tuple(range(n))}


# ---- the decider: seven copies of one of the reference's committed proofs under its key, a word changed in the bad ones ---------------------------------------------
def decider_items():
    """(good, [bad on even places, bad on odd places]): a KZG evaluation + 1 (bit 1 of the single verifier's word), A -> −A (bit 3).  Both pass the parse and the
    per-point stage, so both enter their chunk's equation"""
    from tests import _pairing as bp
    from tests.test_novadecider import _statement
    steps, z0, zf, words = _statement("img2-contrast")

    def changed(at, fn):
        w = list(words)
        w[at] = fn(w[at])
        return (steps, z0, zf, w)

    return (steps, z0, zf, list(words)), [changed(19, lambda v: (v + 1) % bp.R), changed(10, lambda v: bp.Q - v)]


def decider_batch_of(n, bad):
    good, wrong = decider_items()
    return [wrong[i % 2] if i in bad else good for i in range(n)]


def decider_matrix(ctx):
    """every pattern at every chunk and leaf with multipliers from the OS, and with bisection off; nine proofs at chunk 4 whose last chunk is one bad member"""
    from tests import _novadecider as nd
    from vimz_amd.hip import BATCH_STATS, verify_decider_batch, verifying_key_words
    kw = verifying_key_words(nd.verifier_keys()["contrast"])

    def run(items, **kwargs):
        st, sec = {}, {}
        words = verify_decider_batch(ctx, kw, items, stats=st, seconds=sec, **kwargs)
        return {"words": words, "stats": [st[k] for k in BATCH_STATS], "fallback_s": sec["fallback"]}

    out = {}
    for name, bad in patterns(7).items():
        items = decider_batch_of(7, bad)
        for chunk in CHUNKS:
            for leaf in LEAVES:
                out[f"{name}/{chunk}/{leaf}"] = run(items, chunk=chunk, leaf=leaf)
            out[f"{name}/{chunk}/off"] = run(items, chunk=chunk, bisect=False)
    out["nine"] = run(decider_batch_of(9, (1, 8)), chunk=4, leaf=1)
    out["nine/off"] = run(decider_batch_of(9, (1, 8)), chunk=4, bisect=False)
    out["default_leaf"] = run(decider_batch_of(7, (6,)))
    return out


def decider_expected(key):
    """the model's stats for a key of decider_matrix"""
    if key.startswith("nine"):
        roots, bad = R.chunks_of(9, 4), {1: 1, 8: 1}
        return R.stats_without_bisection(roots, bad) if key.endswith("/off") else R.plan(roots, bad, 1)["stats"]
    name, chunk, leaf = key.split("/")
    roots, bad = R.chunks_of(7, int(chunk)), {i: 1 for i in patterns(7)[name]}
    return R.stats_without_bisection(roots, bad) if leaf == "off" else R.plan(roots, bad, int(leaf))["stats"]


# ---- the compressed verifier on a caller's instances ---------------------------------------------------------------------------------------------------------------
INSTANCE_N = (5, 7, 8)
INSTANCE_CHUNKS = (0, 4, 2)
# fixed multipliers: non-trivial 128-bit values, two an instance (never all ones: whoever knows the multipliers can make wrong members cancel)
FIXED_MULTIPLIERS = [((0x9E3779B97F4A7C15F39CC0605CEDC834 * (2 * i + 3)) ^ (0xC2B2AE3D27D4EB4F165667B19E3779F9 >> (i % 7))) % (1 << 128) | (1 << 127) for i in range(2 * max(INSTANCE_N))]


def instance_expected(cid, n, name, chunk, leaf):
    roots, bad = R.chunks_of(n, chunk or 32), {i: 1 << cid for i in patterns(n)[name]}
    return R.stats_without_bisection(roots, bad) if leaf == "off" else R.plan(roots, bad, leaf)["stats"]


def part_instance(ctx, res, orc):
    from tests import _spartan_batch_ref as B
    from tests import _spartan_pub_ref as P
    from tests import _spartan_ref as S
    from tests._oracle import CURVE_SCALAR
    from tests._spartan_batch_gpu import INSTANCE_SHAPES, coos
    from tests._spartan_kernels_gpu import point_words, to_words
    from vimz_amd import hip
    ptr = hip._ptr
    lib = ctx.lib
    lib.vimz_test_spartan_instance_batch_ex.argtypes = [vp, C.c_int, sz, sz, u32, vp, vp, vp, vp, vp, u32, C.c_char_p, sz, vp, vp, vp, vp, sz, vp, vp, C.POINTER(C.c_double), vp,
                                                        u32, sz, C.POINTER(C.c_uint64)]
    lib.vimz_test_spartan_instance_pub_verify.argtypes = [vp, C.c_int, sz, sz, u32, vp, vp, vp, vp, vp, u32, C.c_char_p, vp, C.c_int, vp, sz]
    for cid, shape in INSTANCE_SHAPES.items():
        key = ctx.bases_upload(cid, point_words(S.key_points(cid)))
        try:
            # the relaxed instance of tests/_spartan_batch_gpu.py's part_instance: the strict case's matrices, a random Z, E = Az∘Bz − u·Cz
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
            tail = to_words([u] + X).reshape(-1)
            blobs = {"good": blob, "W": B.bump_final_scalar(c, blob, "W"), "E": B.bump_final_scalar(c, blob, "E")}

            def single(b):
                inst = np.concatenate([np.frombuffer(b[:128], dtype="<u8").astype(np.uint64), tail])
                words = np.frombuffer(b[128:], dtype="<u8").astype(np.uint64)
                return int(lib.vimz_test_spartan_instance_pub_verify(ctx.h, cid, c["n_c"], c["n_w"], len(X), C.byref(A), C.byref(Bm), C.byref(Cm), key.h, ptr(dg), c["side_tag"],
                                                                     P.LABEL, ptr(inst), 1, ptr(words), words.size))

            def batch(kinds, chunk, leaf, mult):
                n = len(kinds)
                inst = np.zeros((n, stride), dtype=np.uint64)
                arrs = []
                for i, k in enumerate(kinds):
                    inst[i, :16] = np.frombuffer(blobs[k][:128], dtype="<u8")
                    inst[i, 16:] = tail
                    arrs.append(np.frombuffer(blobs[k][128:], dtype="<u8").astype(np.uint64))
                wp = (vp * n)(*[a.ctypes.data for a in arrs])
                wn = (sz * n)(*[a.size for a in arrs])
                hE = np.ones(n, dtype=np.int32)
                out = np.full(n, 7, dtype=np.uint32)
                sec = (C.c_double * 6)()
                st = (C.c_uint64 * 4)()
                m = np.ascontiguousarray(to_words(mult[:2 * n])[:, :2]) if mult is not None else None
                ctx._chk(lib.vimz_test_spartan_instance_batch_ex(ctx.h, cid, c["n_c"], c["n_w"], c["n_pub"], C.byref(A), C.byref(Bm), C.byref(Cm), key.h, ptr(dg), c["side_tag"],
                                                                 P.LABEL, n, ptr(inst), ptr(hE), C.cast(wp, vp), C.cast(wn, vp), chunk, ptr(m), ptr(out), sec, None,
                                                                 0 if leaf != "off" else 1, 0 if leaf == "off" else leaf, st))
                return {"results": [int(x) for x in out], "stats": [int(x) for x in st], "fallback_s": sec[5]}

            out = {"single": {k: single(b) for k, b in blobs.items()}, "os": {}, "fixed": {}}
            for n in INSTANCE_N:
                for name, bad in patterns(n).items():
                    kinds = [("W", "E")[i % 2] if i in bad else "good" for i in range(n)]          # wrong-W and wrong-E members mixed
                    for chunk in INSTANCE_CHUNKS:
                        for leaf in LEAVES + ("off",):
                            out["os"][f"{n}/{name}/{chunk}/{leaf}"] = batch(kinds, chunk, leaf, None)
                            if leaf != "off":
                                out["fixed"][f"{n}/{name}/{chunk}/{leaf}"] = batch(kinds, chunk, leaf, FIXED_MULTIPLIERS)
            res[str(cid)] = out
        finally:
            key.free()


# ---- end to end: six Nova + CycleFold proofs of `hash` at HD ------------------------------------------------------------------------------------------------------
def _arg_words(s, t, e):
    return 4 * (3 * s + 4 + 2 * t + 1) + 4 * (4 * t + 1) + (4 * (4 * s + 1) if e else 0)


CF_BAD = {1: 2, 4: 1}          # member 1 (first half): its Grumpkin argument alone; member 4 (second half): a BN254 argument alone


def part_cf(ctx, res):
    from tests.test_circuits import step_inputs
    from vimz_amd import folding
    circuit, params = folding.prepare_folding(ctx, "hash", "HD", backend="sonobe")
    z0, inputs = step_inputs("hash")
    rows = np.stack(inputs)
    pr = folding.fold_input(params, rows[:3], z0, max_batch=4, mode="cyclefold", segments=1)
    try:
        blob, _ = folding.compress_proof(params, pr)
        good = np.array(blob, dtype=np.uint8)
        vk = pr.prover
        hdr = np.frombuffer(good[:64].tobytes(), dtype="<u8")
        s1, t1, s2, t2 = (int(x) for x in hdr[3:7])
        cyclefold_words = _arg_words(s2, t2, True)          # running | fresh | cyclefold: the last argument is the Grumpkin one, the one before it is over BN254

        def flipped(off):
            out = good.copy(); out[off] ^= 1
            return out

        grumpkin_bad, bn254_bad = flipped(len(good) - 32), flipped(len(good) - 8 * cyclefold_words - 32)
        members = [grumpkin_bad if CF_BAD.get(i) == 2 else bn254_bad if CF_BAD.get(i) == 1 else good for i in range(6)]
        single = []
        for b in members:
            try:
                folding.verify_compressed_proof(vk, b, 3, z0)
                single.append(0)
            except Exception as e:          # noqa: BLE001  (the word is in the message)
                single.append(int(str(e).split("flags ")[1].rstrip(")"), 16))
        out = {"single": single}
        for name, kw in (("leaf1", {"leaf": 1}), ("default", {}), ("off", {"bisect": False})):
            st = {}
            words, sec = vk.verify_compressed_batch(members, [3] * 6, [z0] * 6, stats=st, **kw)
            out[name] = {"words": words, "stats": [st[k] for k in ("chunks_refused", "subset_equations", "single_verifications", "accepted_by_subset")], "fallback_s": sec["fallback_s"]}
        st = {}
        out["folding"] = {"words": folding.verify_compressed_proofs(vk, [b.tobytes() for b in members], [3] * 6, [z0] * 6, stats=st), "stats": st}
        res["cf"] = out
    finally:
        pr.close()
        params.free()


def main(part, out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    res = {}
    try:
        if part == "decider":
            res["decider"] = decider_matrix(ctx)
        elif part == "instance":
            from tests import _oracle
            part_instance(ctx, res, _oracle.load())
        elif part == "cf":
            part_cf(ctx, res)
        else:
            raise SystemExit(f"unknown part {part!r}")
    finally:
        ctx.close()
    res["seconds_total"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"batch bisection probe, part {part}: ok, {res['seconds_total']:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
