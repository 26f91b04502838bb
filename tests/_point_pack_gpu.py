"""GPU half of tests/test_gpu_point_pack.py, a process of its own per part with VIMZ_HIP_LIBRARY=testing (`python -m tests._point_pack_gpu {kernels|api|decider}
OUT.json`): packed curve points and packed decider keys (vimz_points_pack / _unpack, vimz_decider_key_pack / _unpack; vimz_amd/csrc/g16_point_pack.hip).

kernels: the two point calls for both groups and both forms over tests/_point_pack_ref.array at every size of SIZES, the identity first, last and everywhere, one
run of VIMZ_PACK_CHUNK + 1 points tiled from a handful, every encoding that must not unpack and every point that must not pack at a known index of a run (the output
prefilled: it must stay), the device's Fq2 root through vimz_test_fq2_sqrt, and the calls' bad arguments.
api: the two key calls on the reference's synthetic keys, short cap, NULLs, truncated input, a tampered point in each part of a key and one exactly on a chunk
boundary of a key of more than a chunk of points, hip's wrappers, every new command with its exit status, and pack_powers / unpack_powers on a contributed string.
decider: once, on the light decider of the hash step (tests/_key_contrib_gpu.DeciderBench): save_key(packed=True) beside save_key(), unpack_key, load_key of the
packed blob with a proof under it, contribute_key on the packed key and verify_key_contributions with either form on either side.
Vectors leave as hex — large ones as the verdict of an exact comparison — and nothing else is judged here.  Test infrastructure."""
import contextlib
import ctypes as C
import io
import json
import sys
import time

import numpy as np

from tests import _key_contrib_ref as K
from tests import _point_pack_ref as ref
from tests._g16_kernels_gpu import hex_of, to_words

FILL = 0xEE


def open_context():
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    vp = C.c_void_p
    for name in ("vimz_points_pack", "vimz_points_unpack"):
        getattr(ctx.lib, name).argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    for name in ("vimz_decider_key_pack", "vimz_decider_key_unpack"):
        getattr(ctx.lib, name).argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint32), vp]
        getattr(ctx.lib, name).restype = C.c_int64
    ctx.lib.vimz_test_fq2_sqrt.argtypes = [vp, vp, C.c_size_t, vp, vp]
    return ctx


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def points_raw(ctx, packing, group, data, form, n=None, null=None, in_place=False, out=None):
    """the C call itself over bytes as they lie in memory: {"rc", "result", "first_bad", "out" (uint8 array), "seconds", "message"}"""
    from vimz_amd import hip
    src = data if isinstance(data, np.ndarray) else u8(data)
    in_size, out_size = ((64, 32) if packing else (32, 64))
    count = src.size // (in_size * group) if n is None else n
    dst = src if in_place else np.full(max(count * out_size * group, 8), FILL, dtype=np.uint8) if out is None else out
    result, first, sec = C.c_uint32(0xFFFF), C.c_uint64(7), (C.c_double * 2)()
    fn = ctx.lib.vimz_points_pack if packing else ctx.lib.vimz_points_unpack
    keep = np.zeros(8, dtype=np.uint8)
    rc = fn(None if null == "ctx" else ctx.h, group, None if null == "in" else hip._ptr(src if src.size else keep), count, form, None if null == "out" else hip._ptr(dst),
            None if null == "result" else C.byref(result), None if null == "first_bad" else C.byref(first), None if null == "seconds" else sec)
    return {"rc": int(rc), "result": int(result.value), "first_bad": int(first.value), "out": dst, "seconds": list(sec),
            "message": ctx.lib.vimz_last_error(ctx.h).decode() if rc and null != "ctx" else ""}


def report(r, size):
    """a small call's result for the JSON: the output as hex, and whether it is still the fill"""
    out = r.pop("out")[:size]
    r["hex"], r["untouched"] = out.tobytes().hex(), bool((out == FILL).all())
    return r


def main_kernels(out_path):
    t_start = time.time()
    from vimz_amd import _lib
    ctx = open_context()
    cn, mg = _lib.FORM_CANONICAL, _lib.FORM_MONTGOMERY
    res = {"pack": {}, "unpack": {}, "reject_unpack": {}, "reject_pack": {}}
    try:
        for group in (1, 2):
            runs = {f"{n}/none": ref.array(group, n) for n in ref.SIZES}
            runs.update({f"65/{ident}": ref.array(group, 65, ident) for ident in ("first", "last", "all")})
            runs["1/all"] = ref.array(group, 1, "all")
            for form, mont in ((cn, 0), (mg, 1)):
                for name, data in runs.items():
                    key = f"g{group}/m{mont}/{name}"
                    p = points_raw(ctx, True, group, ref.to_form(data, mont), form)
                    packed = p["out"].copy()
                    res["pack"][key] = report(p, len(data) // 2)
                    res["unpack"][key] = report(points_raw(ctx, False, group, packed, form), len(data))
            # one run across a chunk boundary: chunk + 1 points tiled from a handful
            chunk = ref.chunk()
            hand = np.frombuffer(ref.array(group, 7, "first"), dtype=np.uint8).reshape(7, 64 * group)
            small = points_raw(ctx, True, group, hand.reshape(-1), cn)
            small_packed = small["out"].reshape(7, 32 * group)
            idx = np.arange(chunk + 1) % 7
            big = np.ascontiguousarray(hand[idx]).reshape(-1)
            p = points_raw(ctx, True, group, big, cn)
            back = points_raw(ctx, False, group, p["out"], cn)
            res[f"chunk_g{group}"] = {"n": chunk + 1, "rc": [p["rc"], back["rc"]], "result": [p["result"], back["result"]], "small_packed": small_packed.tobytes().hex(),
                                     "packed_is_the_tiling": bool(np.array_equal(p["out"].reshape(-1, 32 * group), small_packed[idx])),
                                     "round_trip": bool(np.array_equal(back["out"], big)), "seconds": [p["seconds"], back["seconds"]]}
            # a finding past the boundary: the last point of the run, then also one before it in the first chunk
            spoiled = p["out"].copy()
            bad = ref.bad_packed(group)["x_is_q"][0]
            spoiled[-32 * group:] = u8(bad)
            out = np.full((chunk + 1) * 64 * group, FILL, dtype=np.uint8)
            r1 = points_raw(ctx, False, group, spoiled, cn, out=out)
            spoiled[32 * group * (chunk - 1):32 * group * chunk] = u8(ref.bad_packed(group)["inf_with_sign"][0])
            r2 = points_raw(ctx, False, group, spoiled, cn, out=out)
            res[f"chunk_g{group}"]["spoiled"] = [[r1["rc"], r1["result"], r1["first_bad"]], [r2["rc"], r2["result"], r2["first_bad"]], bool((out == FILL).all())]
            # rejections, each at a known index of a run of 65
            good65 = u8(ref.run(group, True, ref.array(group, 65))[0])
            for k, (name, (data, _f)) in enumerate(ref.bad_packed(group).items()):
                at = (0, 64, 37, 63, 1)[k % 5]
                a = good65.copy()
                a[32 * group * at:32 * group * (at + 1)] = u8(data)
                for form, mont in ((cn, 0), (mg, 1)):
                    r = report(points_raw(ctx, False, group, a, form), 65 * 64 * group)
                    del r["hex"]
                    res["reject_unpack"][f"g{group}/m{mont}/{name}"] = dict(r, at=at)
            pts65 = u8(ref.array(group, 65))
            for k, (name, (data, _f)) in enumerate(ref.bad_points(group).items()):
                at = (64, 0, 38, 63, 2)[k % 5]
                a = pts65.copy()
                a[64 * group * at:64 * group * (at + 1)] = u8(data)
                for form, mont in ((cn, 0), (mg, 1)):
                    r = report(points_raw(ctx, True, group, u8(ref.to_form(a.tobytes(), mont)), form), 65 * 32 * group)
                    del r["hex"]
                    res["reject_pack"][f"g{group}/m{mont}/{name}"] = dict(r, at=at)
            # two findings in one run: the lower index is reported, with its own bits
            a = good65.copy()
            a[32 * group * 40:32 * group * 41] = u8(ref.bad_packed(group)["x_is_q"][0])
            a[32 * group * 9:32 * group * 10] = u8(ref.bad_packed(group)["inf_with_x"][0])
            r = report(points_raw(ctx, False, group, a, cn), 65 * 64 * group)
            res[f"two_findings_g{group}"] = [r["rc"], r["result"], r["first_bad"], r["untouched"]]
        # the device's Fq2 root
        vals = ref.sqrt_values()
        v = to_words([c for a in vals for c in a])
        roots, flags = np.full((len(vals), 8), 7, dtype=np.uint64), np.full(len(vals), 7, dtype=np.uint32)
        from vimz_amd import hip
        rc = ctx.lib.vimz_test_fq2_sqrt(ctx.h, hip._ptr(v), len(vals), hip._ptr(roots), hip._ptr(flags))
        res["fq2_sqrt"] = {"rc": rc, "roots": hex_of(roots), "is_square": [int(x) for x in flags]}
        # bad arguments, n = 0, packing in place
        data = ref.array(1, 5)
        ba = {f"{'pack' if pk else 'unpack'}_null_{x}": points_raw(ctx, pk, 1, data if pk else ref.run(1, True, data)[0], cn, null=x)["rc"] for pk in (True, False) for x in ("ctx", "in", "out", "result", "first_bad")}
        ba.update({"group_0": points_raw(ctx, True, 0, data, cn, n=5)["rc"], "group_3": points_raw(ctx, False, 3, data, cn, n=5)["rc"], "form_7": points_raw(ctx, True, 1, data, 7)["rc"],
                   "unpack_in_place": points_raw(ctx, False, 1, u8(data), cn, n=5, in_place=True)["rc"]})
        buf = np.zeros(64 * 5 + 32, dtype=np.uint8)
        buf[32:] = u8(data)
        from_mid = points_raw(ctx, True, 1, buf[32:], cn, out=buf[:160])      # the output's end overlaps the input's start
        ba["pack_overlapping"] = from_mid["rc"]
        res["bad_arguments"] = ba
        res["null_seconds"] = report(points_raw(ctx, True, 1, data, cn, null="seconds"), 160)
        res["n_zero"] = [report(points_raw(ctx, pk, g, b"", cn, n=0), 8) for pk in (True, False) for g in (1, 2)]
        same = points_raw(ctx, True, 2, u8(ref.array(2, 9, "last")), cn, in_place=True)
        res["pack_in_place"] = {"rc": same["rc"], "result": same["result"], "hex": same["out"][:9 * 64].tobytes().hex()}
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"point pack kernels probe ok: {len(res['pack'])} runs each way, {len(res['reject_unpack']) + len(res['reject_pack'])} rejections, chunk runs "
          f"{res['chunk_g1']['seconds']} / {res['chunk_g2']['seconds']} s, {res['seconds']:.1f} s")


def key_raw(ctx, packing, blob, cap=None, null=None, in_place=False):
    """the C call itself: {"rc", "result", "first_bad", "hex", "untouched", "message"}"""
    from vimz_amd import hip
    src = blob if isinstance(blob, np.ndarray) else u8(blob)
    size = ref.packed_size(src.size) if packing else 2 * (src.size - 88) + 88
    dst = np.full(max(size, src.size, 8), FILL, dtype=np.uint8)
    if in_place:
        dst[:src.size] = src
        src = dst[:src.size]
    result, first = C.c_uint32(0xFFFF), np.full(2, 7, dtype=np.uint64)
    fn = ctx.lib.vimz_decider_key_pack if packing else ctx.lib.vimz_decider_key_unpack
    rc = fn(None if null == "ctx" else ctx.h, None if null == "in" else hip._ptr(src if src.size else np.zeros(8, dtype=np.uint8)), src.size, None if null == "out" else hip._ptr(dst),
            dst.size if cap is None else cap, None if null == "result" else C.byref(result), None if null == "first_bad" else hip._ptr(first))
    return {"rc": int(rc), "result": int(result.value), "first_bad": [int(first[0]), int(first[1])], "out": dst[:max(size, 0)], "untouched": bool(in_place or (dst == FILL).all()),
            "message": ctx.lib.vimz_last_error(ctx.h).decode() if rc < 0 and null != "ctx" else ""}


def small(r):
    r["hex"] = r.pop("out").tobytes().hex()
    return r


def big_key(n_g1_over):
    """a key blob of more than a chunk of G1 points, tiled from a handful: (blob, runs)"""
    m = (ref.chunk() + n_g1_over) // 3 + 1
    shape = (m, 1, 4)
    L = ref.runs(*shape)
    head = b"".join(x.to_bytes(8, "little") for x in (K.KEY_MAGIC, m, 1, 2, 4, 1, 1)) + bytes(32)
    fixed = b"".join(ref.point_bytes(g, 11 + k) for k, (g, _o, _p) in enumerate(ref.FIXED))
    g1 = np.frombuffer(ref.array(1, 7, "first"), dtype=np.uint8).reshape(7, 64)
    g2 = np.frombuffer(ref.array(2, 5, "last"), dtype=np.uint8).reshape(5, 128)
    blob = np.concatenate([u8(head + fixed), g1[np.arange(L["n_g1"]) % 7].reshape(-1), g2[np.arange(L["n_g2"]) % 5].reshape(-1)])
    assert blob.size == 8 * L["words"]
    return blob, L


def main_api(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip, iden3
    ctx = open_context()
    res = {}
    try:
        # the two key calls beside the reference's bytes
        res["keys"] = {}
        for name, (shape, identity) in {"small": (K.SMALL, None), "small_identity": (K.SMALL, 3), "large": (K.LARGE, None), "large_identity": (K.LARGE, 3)}.items():
            key = K.synthetic_key(K.DELTA0, shape, identity)
            p = key_raw(ctx, True, key)
            packed = p["out"].copy()
            res["keys"][name] = {"pack": small(p), "unpack": small(key_raw(ctx, False, packed)), "pack_in_place": small(key_raw(ctx, True, key, in_place=True)),
                                 "unpack_in_place": small(key_raw(ctx, False, packed, in_place=True))}
        key = K.synthetic_key(K.DELTA0, K.LARGE)
        packed = ref.pack_key(key)[0]
        res["short_cap"] = {"pack": small(key_raw(ctx, True, key, cap=len(packed) - 1)), "unpack": small(key_raw(ctx, False, packed, cap=len(key) - 1)),
                            "pack_no_out": key_raw(ctx, True, key, null="out")["rc"], "unpack_no_out": key_raw(ctx, False, packed, null="out")["rc"], "sizes": [len(packed), len(key)]}
        ba = {f"{'pack' if pk else 'unpack'}_null_{x}": key_raw(ctx, pk, key if pk else packed, null=x)["rc"] for pk in (True, False) for x in ("ctx", "in", "result", "first_bad")}
        refused = {"pack_truncated": key_raw(ctx, True, key[:-8]), "pack_oversized": key_raw(ctx, True, key + bytes(8)), "pack_a_packed_key": key_raw(ctx, True, packed),
                   "unpack_truncated": key_raw(ctx, False, packed[:-8]), "unpack_oversized": key_raw(ctx, False, packed + bytes(8)), "unpack_a_plain_key": key_raw(ctx, False, key),
                   "unpack_one_byte": key_raw(ctx, False, packed[:1]), "unpack_wrong_magic": key_raw(ctx, False, K.put(packed, 0, b"VG16KPK2"))}
        res["refused"] = {k: {"rc": r["rc"], "message": r["message"], "untouched": r["untouched"]} for k, r in refused.items()}
        res["bad_arguments"] = ba
        # a tampered point in each part
        res["tampered"] = {}
        for name, (group, off, poff) in ref.key_point_words(K.LARGE).items():
            y = off + 8 * group - 4
            bad = K.put(key, y, ((K.coord(key, y) + 1) % K.Q).to_bytes(32, "little"))
            badp = K.put(packed, poff + 4 * group - 4, K.Q.to_bytes(32, "little"))
            res["tampered"][name] = {"pack": small(key_raw(ctx, True, bad)), "unpack": small(key_raw(ctx, False, badp))}
        # ... and exactly on a chunk boundary
        blob, L = big_key(5)
        chunk = ref.chunk()
        clean = key_raw(ctx, True, blob)
        back = key_raw(ctx, False, clean["out"])
        bd = {"n_g1": L["n_g1"], "chunk": chunk, "clean": [clean["rc"], clean["result"], back["rc"], back["result"]], "round_trip": bool(np.array_equal(back["out"], blob)),
              "bytes": [int(blob.size), int(clean["out"].size)], "pack": {}, "unpack": {}}
        for label, i in (("last_of_chunk_0", chunk - 1), ("first_of_chunk_1", chunk), ("last_g1", L["n_g1"] - 1)):
            w = L["off_g1"] + 8 * i
            bad = blob.copy()
            bad[8 * (w + 4):8 * (w + 8)] = u8(((int.from_bytes(blob[8 * (w + 4):8 * (w + 8)].tobytes(), "little") + 1) % K.Q).to_bytes(32, "little")) if i % 7 else u8((5).to_bytes(32, "little"))
            r = key_raw(ctx, True, bad)
            bd["pack"][label] = [r["rc"], r["result"], r["first_bad"], r["untouched"], w]
            pw = L["poff_g1"] + 4 * i
            badp = clean["out"].copy()
            badp[8 * pw:8 * (pw + 4)] = u8(K.Q.to_bytes(32, "little"))
            r = key_raw(ctx, False, badp)
            bd["unpack"][label] = [r["rc"], r["result"], r["first_bad"], r["untouched"], pw]
        res["boundary"] = bd
        # hip's wrappers
        pts = np.frombuffer(ref.array(2, 9, "first"), dtype="<u8").reshape(9, 16)
        sec = []
        pk = hip.pack_points(ctx, 2, pts, seconds=sec)
        py = {"pack_points": hex_of(pk), "shape": list(pk.shape), "unpack_points": hex_of(hip.unpack_points(ctx, 2, pk)), "seconds": list(sec),
              "empty": [list(hip.pack_points(ctx, 1, np.zeros((0, 8), dtype=np.uint64)).shape), list(hip.unpack_points(ctx, 1, np.zeros((0, 4), dtype=np.uint64)).shape)]}
        pkey = hip.pack_key(ctx, key)
        py.update({"pack_key": pkey.tobytes().hex(), "unpack_key": hip.unpack_key(ctx, pkey).tobytes().hex(), "key_is_packed": [hip.key_is_packed(pkey), hip.key_is_packed(key), hip.key_is_packed(b"")],
                   "problems": hip.pack_problems(ref.COORD | ref.OFF_CURVE)})
        origin, final, records = K.chain(K.LARGE, 1)
        k1, r1 = hip.contribute_key(ctx, hip.pack_key(ctx, origin), delta=K.DELTAS[0], nonce=K.NONCES[0])
        py["contribute_packed"] = {"is_packed": hip.key_is_packed(k1), "key": k1.tobytes().hex(), "record": r1.tobytes().hex()}
        py["verify_mixed"] = [hip.verify_key_contributions(ctx, o, f, records) for o in (origin, hip.pack_key(ctx, origin)) for f in (final, hip.pack_key(ctx, final))]
        refusals = {}
        bad_pk = pk.copy(); bad_pk[4, 7] |= np.uint64(1 << 62); bad_pk[4, 7] |= np.uint64(1 << 63)
        for name, fn in (("unpack_points", lambda: hip.unpack_points(ctx, 2, bad_pk)), ("pack_points_group", lambda: hip.pack_points(ctx, 3, pts)),
                         ("pack_key", lambda: hip.pack_key(ctx, K.put(key, ref.KEY_IC + 4, (K.coord(key, ref.KEY_IC + 4) ^ 1).to_bytes(32, "little")))),
                         ("unpack_key_not_packed", lambda: hip.unpack_key(ctx, key))):
            try:
                fn(); refusals[name] = [0, ""]
            except _lib.VimzError as e:
                refusals[name] = [e.code, str(e)]
        py["refusals"] = refusals
        res["python"] = py
        # the strings
        powers = iden3.new_powers(3)
        powers, _rec = hip.contribute_powers(ctx, powers)
        blob_p = iden3.pack_powers(ctx, powers)
        back_p = iden3.unpack_powers(ctx, blob_p)
        ptau = iden3.write_ptau(powers)
        res["powers"] = {"bytes": [len(blob_p), len(ptau)], "magic": blob_p[:8].decode(), "head": list(blob_p[8:16]), "same_file": iden3.write_ptau(back_p) == ptau,
                         "tau_g1_1": [blob_p[16 + 32:16 + 64].hex(), np.ascontiguousarray(powers["tau_g1"][1]).tobytes().hex()], "verify": hip.verify_powers(ctx, back_p)}
        prefusals = {}
        for name, fn in (("truncated", lambda: iden3.unpack_powers(ctx, blob_p[:-8])), ("magic", lambda: iden3.unpack_powers(ctx, b"VPOTPK02" + blob_p[8:])),
                         ("bad_point", lambda: iden3.unpack_powers(ctx, blob_p[:16 + 31] + b"\xc0" + blob_p[16 + 32:]))):
            try:
                fn(); prefusals[name] = "accepted"
            except ValueError as e:
                prefusals[name] = "ValueError: " + str(e)
            except _lib.VimzError as e:
                prefusals[name] = f"VimzError {e.code}: {e}"
        res["powers"]["refusals"] = prefusals
        # every new command
        paths = {x: f"{out_path}.{x}" for x in ("plain.key", "packed.key", "back.key", "one.key", "records", "in.ptau", "packed.pot", "back.ptau")}
        with open(paths["plain.key"], "wb") as fp:
            fp.write(origin)
        with open(paths["in.ptau"], "wb") as fp:
            fp.write(ptau)
        res["cli"] = {}
        for name, argv in (("pack_key", ["pack-key", paths["plain.key"], paths["packed.key"]]), ("unpack_key", ["unpack-key", paths["packed.key"], paths["back.key"]]),
                           ("contribute_packed", ["contribute", paths["packed.key"], paths["one.key"], paths["records"]]),
                           ("verify_plain_origin", ["verify-contributions", paths["plain.key"], paths["one.key"], paths["records"]]),
                           ("verify_packed_origin", ["verify-contributions", paths["packed.key"], paths["one.key"], paths["records"]]),
                           ("pack_powers", ["pack-powers", paths["in.ptau"], paths["packed.pot"]]), ("unpack_powers", ["unpack-powers", paths["packed.pot"], paths["back.ptau"]]),
                           ("usage_pack_key", ["pack-key", paths["plain.key"]]), ("usage_unpack_key", ["unpack-key"]), ("usage_pack_powers", ["pack-powers", paths["in.ptau"]]),
                           ("usage_unpack_powers", ["unpack-powers", "a", "b", "c"])):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
                rc = iden3._main(argv)
            res["cli"][name] = {"rc": rc, "stdout": buf.getvalue()}
        read = lambda p: open(p, "rb").read()      # noqa: E731
        res["cli"]["files"] = {"packed_key": read(paths["packed.key"]) == ref.pack_key(origin)[0], "back_key": read(paths["back.key"]) == origin,
                               "one_key_is_packed": read(paths["one.key"])[:8] == b"VG16KPK1", "packed_powers": read(paths["packed.pot"]) == blob_p, "back_ptau": read(paths["back.ptau"]) == ptau}
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                res["cli"]["unpack_a_plain_key"] = iden3._main(["unpack-key", paths["plain.key"], paths["back.key"]])
        except _lib.VimzError as e:
            res["cli"]["unpack_a_plain_key"] = f"VimzError {e.code}"
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"point pack api probe ok: {len(res['keys'])} keys, {len(res['tampered'])} tampered parts, boundary key of {res['boundary']['n_g1']} G1 points, {res['seconds']:.1f} s")


def main_decider(out_path):
    t_start = time.time()
    from tests._key_contrib_gpu import DELTA, STEPS, DeciderBench
    from tests._key_contrib_gpu import open_context as open_key_context
    from vimz_amd import _lib, hip
    ctx, fixed_mul = open_key_context()
    res = {}
    bench = DeciderBench(ctx, fixed_mul)
    try:
        d0 = bench.trapdoor_decider(DELTA)
        res["info"] = d0.info()
        t0 = time.time()
        plain = d0.save_key()
        t1 = time.time()
        packed = d0.save_key(packed=True)
        t2 = time.time()
        back = hip.unpack_key(ctx, packed)
        t3 = time.time()
        res["sizes"] = {"plain": int(plain.size), "packed": int(packed.size)}
        res["wall_seconds"] = {"save_key": t1 - t0, "save_key_packed": t2 - t1, "unpack_key": t3 - t2}
        res["is_packed"] = [hip.key_is_packed(packed), hip.key_is_packed(plain)]
        res["unpack_is_save_key"] = bool(np.array_equal(back, plain))
        res["pack_of_unpack"] = bool(np.array_equal(hip.pack_key(ctx, back), packed))
        d0.close()
        d1 = hip.Decider.load_key(bench.cf, packed)
        try:
            words, pub, _ = d1.prove()
            lz = bench.circuit.len_z
            z0, zi = pub[2:2 + lz], pub[2 + lz:2 + 2 * lz]
            res["proof"] = {"verify": d1.verify(STEPS, z0, zi, words), "light": d1.light, "info": d1.info(), "verify_wrong_steps": d1.verify(STEPS + 1, z0, zi, words)}
        finally:
            d1.close()
        got, rec = hip.contribute_key(ctx, packed, delta=K.DELTAS[0] % K.R, nonce=K.NONCES[0])
        got_plain, rec_plain = hip.contribute_key(ctx, plain, delta=K.DELTAS[0] % K.R, nonce=K.NONCES[0])
        res["contribute"] = {"is_packed": [hip.key_is_packed(got), hip.key_is_packed(got_plain)], "same_key": bool(np.array_equal(hip.unpack_key(ctx, got), got_plain)),
                             "same_record": rec.tobytes() == rec_plain.tobytes(), "bytes": [int(got.size), int(got_plain.size)]}
        res["chains"] = {f"{'packed' if o is packed else 'plain'}_{'packed' if f is got else 'plain'}": hip.verify_key_contributions(ctx, o, f, rec) for o in (plain, packed) for f in (got_plain, got)}
        res["chain_against_itself"] = hip.verify_key_contributions(ctx, packed, packed, rec)
    finally:
        bench.close()
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"point pack decider probe ok: domain {res['info']['domain']}, key {res['sizes']['plain']} -> {res['sizes']['packed']} bytes, wall seconds {res['wall_seconds']}, {res['seconds']:.1f} s in all")


if __name__ == "__main__":
    {"kernels": main_kernels, "api": main_api, "decider": main_decider}[sys.argv[1]](sys.argv[2])
