"""GPU half of tests/test_gpu_key_contrib.py, a process of its own per part with VIMZ_HIP_LIBRARY=testing (`python -m tests._key_contrib_gpu {kernels|api|decider}
OUT.json`): further delta contributions to a saved decider key (vimz_decider_key_contribute, vimz_decider_key_verify_contributions; vimz_amd/csrc/g16_key_contrib.hip).

kernels: k_ratio_rlc and its reduction through vimz_test_ratio_rlc over the cases of tests/_key_contrib_ref.ratio_cases().  Points are [s_i]G made by
vimz_test_g16_fixed_mul, the expected sums [Σ rho_i·s_i]G made the same way; the two-launch form of the testing hook runs over three of the cases too.
api: the two calls on the reference's synthetic keys — contribute with a fixed delta' and nonce beside the Python reference's bytes (also in place, and with a short
cap), verify over chains of 0, 1 and 3 records and over every tampered chain, contribute's refusals, verify's bad arguments, the production entry (delta' from the
OS), hip's wrappers and the two commands of `python -m vimz_amd.iden3`.
decider: once, on the light decider of the hash step (domain 2^18): the trapdoor set-up's key of delta contributed to with delta' beside the trapdoor set-up's key of
delta·delta', the chain's verdict, a proof under the loaded contributed key, and the commands on those files.
measure (not run by the tests; what profiles/key_contrib.txt records): contribute's and verify's stage times on that key and the combination in both forms,
alternating, through vimz_test_ratio_rlc_forms; `measure full` the same on the full decider of contrast HD.
Vectors leave as hex and nothing is judged here.  Test infrastructure."""
import contextlib
import ctypes as C
import io
import json
import sys
import time

import numpy as np

from tests import _key_contrib_ref as K
from tests._g16_kernels_gpu import hex_of, to_words
from tests._pairing import R

TAU, ALPHA, BETA, DELTA = 0x2545F4914F6CDD1D0123456789ABCDEF, 0xFEDCBA987654321, 0x55AA55AA55AA77, 0x1B873593CC9E2D51
N_SRS, STEPS = 36000, 4
TWO_LAUNCH_CASES = ("19/multiple", f"{K.PT_BLOCK * K.RLC_CHUNK + 1}/multiple", "1030/unrelated")


def open_context():
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    vp = C.c_void_p
    ctx.lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    ctx.lib.vimz_test_ratio_rlc.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int, vp]
    ctx.lib.vimz_test_ratio_rlc_forms.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    ctx.lib.vimz_decider_key_contribute.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(C.c_double)]
    ctx.lib.vimz_decider_key_contribute.restype = C.c_int64
    ctx.lib.vimz_testing_decider_key_contribute_delta.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, C.POINTER(C.c_double)]
    ctx.lib.vimz_testing_decider_key_contribute_delta.restype = C.c_int64
    ctx.lib.vimz_decider_key_verify_contributions.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint32), vp, C.POINTER(C.c_double)]

    def fixed_mul(group, scalars):
        out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
        ctx._chk(ctx.lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(to_words(scalars)), len(scalars), hip._ptr(out)))
        return out
    return ctx, fixed_mul


def rho_words(rho):
    return np.frombuffer(b"".join(x.to_bytes(16, "little") for x in rho), dtype="<u8").astype(np.uint64)


def main_kernels(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    ctx, fixed_mul = open_context()
    cn = _lib.FORM_CANONICAL
    res = {"ratio": {}, "two_launches": {}}
    try:
        cases = K.ratio_cases()
        want = []
        for name, (before, after, rho) in cases.items():
            n = len(rho)
            b, a, rw = fixed_mul(1, before), fixed_mul(1, after), rho_words(rho)
            out = np.full((2, 8), 7, dtype=np.uint64)
            t0 = time.time()
            ctx._chk(ctx.lib.vimz_test_ratio_rlc(ctx.h, hip._ptr(b), hip._ptr(a), n, hip._ptr(rw), cn, hip._ptr(out)))
            res["ratio"][name] = {"out": hex_of(out), "seconds": time.time() - t0}
            if name in TWO_LAUNCH_CASES:
                out2 = np.full((2, 8), 7, dtype=np.uint64)
                ctx._chk(ctx.lib.vimz_test_ratio_rlc_forms(ctx.h, hip._ptr(b), hip._ptr(a), n, hip._ptr(rw), cn, 2, 1, hip._ptr(out2), None))
                res["two_launches"][name] = hex_of(out2)
            want += list(K.ratio_scalars(before, after, rho))
        pts = fixed_mul(1, want)
        for k, name in enumerate(cases):
            res["ratio"][name]["want"] = hex_of(pts[2 * k:2 * k + 2])
        # the Montgomery form of the same call, and its bad arguments
        before, after, rho = cases["19/multiple"]
        mont = lambda arr: np.frombuffer(b"".join((int.from_bytes(arr.tobytes()[i:i + 32], "little") * (1 << 256) % K.Q).to_bytes(32, "little") for i in range(0, arr.nbytes, 32)),      # noqa: E731
                                         dtype="<u8").astype(np.uint64)
        b, a, out = fixed_mul(1, before), fixed_mul(1, after), np.full((2, 8), 7, dtype=np.uint64)
        ctx._chk(ctx.lib.vimz_test_ratio_rlc(ctx.h, hip._ptr(mont(b)), hip._ptr(mont(a)), 19, hip._ptr(rho_words(rho)), _lib.FORM_MONTGOMERY, hip._ptr(out)))
        res["montgomery"] = {"out": hex_of(out), "want": hex_of(mont(pts[2 * list(cases).index("19/multiple"):][:2]))}
        off = b.copy(); off[4, 4] ^= np.uint64(1)
        res["bad_arguments"] = {"n_0": ctx.lib.vimz_test_ratio_rlc(ctx.h, hip._ptr(b), hip._ptr(a), 0, hip._ptr(rho_words(rho)), cn, hip._ptr(out)),
                                "form_7": ctx.lib.vimz_test_ratio_rlc(ctx.h, hip._ptr(b), hip._ptr(a), 19, hip._ptr(rho_words(rho)), 7, hip._ptr(out)),
                                "null_after": ctx.lib.vimz_test_ratio_rlc(ctx.h, hip._ptr(b), None, 19, hip._ptr(rho_words(rho)), cn, hip._ptr(out)),
                                "off_curve": ctx.lib.vimz_test_ratio_rlc(ctx.h, hip._ptr(off), hip._ptr(a), 19, hip._ptr(rho_words(rho)), cn, hip._ptr(out))}
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"key contribution kernels probe ok: {len(res['ratio'])} combinations, {res['seconds']:.1f} s")


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def contribute_raw(ctx, blob, delta=None, nonce=None, in_place=False, cap=None, null=None):
    """the C call itself: {"rc", "key" (hex), "record" (hex), "message"}"""
    from vimz_amd import hip
    src = u8(blob)
    dst = src if in_place else np.full(src.size, 0xEE, dtype=np.uint8)
    rec, sec = np.full(37, 7, dtype=np.uint64), (C.c_double * 3)()
    args = [None if null == "ctx" else ctx.h, None if null == "key_in" else hip._ptr(src), src.size, None if null == "key_out" else hip._ptr(dst), dst.size if cap is None else cap,
            None if null == "record" else hip._ptr(rec)]
    if delta is None:
        rc = ctx.lib.vimz_decider_key_contribute(*args, sec)
    else:
        rc = ctx.lib.vimz_testing_decider_key_contribute_delta(*args, hip._ptr(to_words([delta])), hip._ptr(to_words([nonce])), sec)
    return {"rc": int(rc), "key": dst.tobytes().hex(), "record": rec.tobytes().hex(), "seconds": list(sec), "message": ctx.lib.vimz_last_error(ctx.h).decode() if rc < 0 and null != "ctx" else ""}


def verify_raw(ctx, origin, final, records, null=None, n_records=None):
    from vimz_amd import hip
    o, f, r = u8(origin), u8(final), u8(records)
    result, first, sec = C.c_uint32(0xFFFF), np.full(2, 7, dtype=np.uint64), (C.c_double * 4)()
    rc = ctx.lib.vimz_decider_key_verify_contributions(None if null == "ctx" else ctx.h, None if null == "origin" else hip._ptr(o), o.size, None if null == "final" else hip._ptr(f), f.size,
                                                       hip._ptr(r) if r.size and null != "records" else None, r.size // K.RECORD_BYTES if n_records is None else n_records,
                                                       None if null == "result" else C.byref(result), None if null == "first_bad" else hip._ptr(first), None if null == "seconds" else sec)
    return {"rc": rc, "result": int(result.value), "first_bad": [int(first[0]), int(first[1])], "seconds": list(sec), "message": ctx.lib.vimz_last_error(ctx.h).decode() if rc and null != "ctx" else ""}


def main_api(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip, iden3
    ctx, _fixed_mul = open_context()
    res = {}
    try:
        # contribute beside the reference, byte for byte
        res["contribute"] = {}
        for name, (shape, identity) in {"small": (K.SMALL, None), "small_identity_in_l": (K.SMALL, 2), "large": (K.LARGE, None)}.items():
            key = K.synthetic_key(K.DELTA0, shape, identity)
            want_key, want_rec = K.contribute(key, K.DELTAS[0], K.NONCES[0])
            got = contribute_raw(ctx, key, K.DELTAS[0], K.NONCES[0])
            same = contribute_raw(ctx, key, K.DELTAS[0], K.NONCES[0], in_place=True)
            res["contribute"][name] = {"rc": got["rc"], "bytes": len(key), "key": got["key"] == want_key.hex(), "record": got["record"] == want_rec.hex(),
                                       "in_place_rc": same["rc"], "in_place_key": same["key"] == want_key.hex(), "in_place_record": same["record"] == want_rec.hex(), "seconds": got["seconds"]}
        key = K.synthetic_key(K.DELTA0, K.LARGE)
        short = contribute_raw(ctx, key, K.DELTAS[0], K.NONCES[0], cap=len(key) - 1)
        res["short_cap"] = {"rc": short["rc"], "untouched": short["key"] == "ee" * len(key), "no_key_out": contribute_raw(ctx, key, K.DELTAS[0], K.NONCES[0], null="key_out")["rc"], "bytes": len(key)}
        # the chains
        res["accepted"] = {str(n): verify_raw(ctx, *K.chain(K.LARGE, n)) for n in (0, 1, 3)}
        res["accepted"]["small_identity_in_l"] = verify_raw(ctx, *K.chain(K.SMALL, 1, 2))
        res["accepted"]["null_seconds"] = verify_raw(ctx, *K.chain(K.LARGE, 1), null="seconds")
        res["tampered"] = {name: verify_raw(ctx, *chain) for name, chain in K.tampered_chains(K.LARGE).items()}
        origin, final, records = K.chain(K.LARGE, 3)
        res["other_sizes"] = verify_raw(ctx, origin, K.synthetic_key(K.DELTA0, K.SMALL), records)
        res["refused"] = {name: contribute_raw(ctx, blob, K.DELTAS[0], K.NONCES[0]) for name, (blob, _msg) in K.refused_keys(K.LARGE).items()}
        for r in res["refused"].values():
            del r["key"], r["record"]
        res["refused_product_entry"] = contribute_raw(ctx, K.refused_keys(K.LARGE)["truncated"][0])["rc"]
        res["bad_arguments"] = {f"contribute_null_{x}": contribute_raw(ctx, key, K.DELTAS[0], K.NONCES[0], null=x)["rc"] for x in ("ctx", "key_in", "record")}
        res["bad_arguments"].update({f"verify_null_{x}": verify_raw(ctx, origin, final, records, null=x)["rc"] for x in ("ctx", "origin", "final", "records", "result", "first_bad")})
        res["bad_arguments"].update({"verify_truncated_origin": verify_raw(ctx, origin[:-8], final, records)["rc"], "verify_oversized_final": verify_raw(ctx, origin, final + bytes(8), records)["rc"],
                                     "verify_record_magic": verify_raw(ctx, origin, final, K.put(records, K.RECORD_WORDS, b"VG16CTR2"))["rc"],
                                     "delta_zero": contribute_raw(ctx, key, 0, 5)["rc"], "delta_is_r": contribute_raw(ctx, key, R, 5)["rc"]})
        # the production entry: delta' from the OS, twice
        a, b = contribute_raw(ctx, origin), None
        b = contribute_raw(ctx, bytes.fromhex(a["key"]))
        two = bytes.fromhex(a["record"]) + bytes.fromhex(b["record"])
        res["os_delta"] = {"rc": [a["rc"], b["rc"]], "keys_differ": a["key"] != origin.hex() and a["key"] != b["key"], "records_differ": a["record"] != b["record"],
                           "chain": verify_raw(ctx, origin, bytes.fromhex(b["key"]), two), "first_alone": verify_raw(ctx, origin, bytes.fromhex(a["key"]), two[:K.RECORD_BYTES]),
                           "fixed_part_kept": K.put(K.put(K.put(bytes.fromhex(b["key"]), K.KEY_DELTA1, bytes(64)), K.KEY_DELTA2, bytes(128)), K.layout(origin)["off_lh"], bytes(64 * 19))
                           == K.put(K.put(K.put(origin, K.KEY_DELTA1, bytes(64)), K.KEY_DELTA2, bytes(128)), K.layout(origin)["off_lh"], bytes(64 * 19))}
        # hip's wrappers and the command line
        k1, r1 = hip.contribute_key(ctx, origin, delta=K.DELTAS[0], nonce=K.NONCES[0])
        sec = []
        res["python"] = {"key": k1.tobytes() == K.chain(K.LARGE, 1)[1], "record": r1.tobytes() == K.chain(K.LARGE, 1)[2], "verify": hip.verify_key_contributions(ctx, origin, k1, r1, seconds=sec),
                         "seconds": list(sec), "verify_bytes": hip.verify_key_contributions(ctx, origin, final, records), "problems": hip.keychain_problems(K.LAST | K.RATIO),
                         "tampered": hip.verify_key_contributions(ctx, *K.tampered_chains(K.LARGE)["record_z_off_by_one"])}
        refusals = {}
        for name, fn in (("delta_without_nonce", lambda: hip.contribute_key(ctx, origin, delta=5)), ("records_length", lambda: hip.verify_key_contributions(ctx, origin, final, records[:-1])),
                         ("not_a_key", lambda: hip.contribute_key(ctx, origin[:-8]))):
            try:
                fn(); refusals[name] = [0, ""]
            except _lib.VimzError as e:
                refusals[name] = [e.code, str(e)]
        res["python"]["refusals"] = refusals
        paths = {x: f"{out_path}.{x}" for x in ("origin.key", "one.key", "two.key", "records", "bad.key")}
        with open(paths["origin.key"], "wb") as fp:
            fp.write(origin)
        with open(paths["bad.key"], "wb") as fp:
            fp.write(K.tampered_chains(K.LARGE)["l_h_point_scaled/second_chunk"][1])
        res["cli"] = {}
        for name, argv in (("contribute_1", ["contribute", paths["origin.key"], paths["one.key"], paths["records"]]), ("contribute_2", ["contribute", paths["one.key"], paths["two.key"], paths["records"]]),
                           ("verify_2", ["verify-contributions", paths["origin.key"], paths["two.key"], paths["records"]]), ("verify_wrong_final", ["verify-contributions", paths["origin.key"], paths["one.key"], paths["records"]]),
                           ("verify_bad_key", ["verify-contributions", paths["origin.key"], paths["bad.key"], paths["records"]]), ("usage_contribute", ["contribute", paths["origin.key"]]),
                           ("usage_verify", ["verify-contributions"])):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
                rc = iden3._main(argv)
            res["cli"][name] = {"rc": rc, "stdout": buf.getvalue()}
        with open(paths["records"], "rb") as fp:
            res["cli"]["records_bytes"] = len(fp.read())
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"key contribution api probe ok: {len(res['tampered'])} tampered chains, {res['seconds']:.1f} s")


class DeciderBench:
    """a prover over the hash step (or contrast) at HD with STEPS folds, and deciders by the trapdoor set-up hook with a given delta"""

    def __init__(self, ctx, fixed_mul, transformation="hash", light=True):
        from tests.test_circuits import step_inputs
        from vimz_amd import _lib, hip
        from vimz_amd.circuit import Circuit
        self.ctx, self.light = ctx, light
        self.circuit = Circuit.for_resolution(transformation, "HD")
        self.z0, inputs = step_inputs(transformation)
        self.ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
        from vimz_amd import folding
        # the SRS: the hash step's as the other decider probes size it; any other step's as prepare_folding sizes a key
        n_srs = N_SRS if transformation == "hash" else 1 << (max(self.circuit.n_wires, self.circuit.n_constraints) + folding.CYCLEFOLD_ROOM - 1).bit_length()
        self.srs = ctx.bases_upload(_lib.CURVE_BN254_G1, fixed_mul(1, [pow(TAU, k, R) for k in range(n_srs)]))
        self.vk = fixed_mul(2, [TAU]).reshape(4, 4)
        self.cf = hip.CycleFoldIVC(ctx, self.circuit, self.srs, self.ck2, max_batch=2)
        self.cf.reset(self.z0); self.cf.fold(np.stack(inputs[:STEPS]))

    def trapdoor_decider(self, delta):
        from vimz_amd import hip
        vp = C.c_void_p
        fn = self.ctx.lib.vimz_testing_decider_setup_trapdoor
        fn.argtypes = [vp, vp, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_double)]
        h, sec4 = vp(), (C.c_double * 4)()
        self.ctx._chk(fn(self.cf.h, hip._ptr(self.vk), int(self.light), hip._ptr(to_words([TAU, ALPHA, BETA, 1, delta])), C.byref(h), sec4))
        d = hip.Decider.__new__(hip.Decider)      # (as Decider.load_key wraps a handle)
        d.prover, d.ctx, d.h, d.light = self.cf, self.ctx, h, self.light
        lib = self.ctx.lib
        lib.vimz_decider_free.argtypes, lib.vimz_decider_free.restype, lib.vimz_decider_info.argtypes = [vp], None, [vp, vp]
        lib.vimz_decider_vk.argtypes, lib.vimz_decider_vk.restype = [vp, vp, C.c_size_t], C.c_int64
        lib.vimz_decider_prove.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_double)]
        lib.vimz_decider_verify.argtypes = [vp, C.c_uint64, vp, vp, vp, C.POINTER(C.c_uint32)]
        return d

    def close(self):
        self.cf.close(); self.srs.free(); self.ck2.free()


def main_decider(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip, iden3
    ctx, fixed_mul = open_context()
    res = {}
    bench = DeciderBench(ctx, fixed_mul)
    dp = K.DELTAS[0] % R
    try:
        d0 = bench.trapdoor_decider(DELTA)
        res["info"] = d0.info()
        origin = d0.save_key()
        d1 = bench.trapdoor_decider(DELTA * dp % R)
        want = d1.save_key()
        d1.close()
        sec_c, sec_v = [], []
        got, rec = hip.contribute_key(ctx, origin, delta=dp, nonce=K.NONCES[0], seconds=sec_c)
        res["key"] = {"bytes": [int(origin.size), int(got.size), int(want.size)], "identical": bool(np.array_equal(got, want)), "origin_differs": not np.array_equal(got, origin),
                      "first_difference": None if got.size != want.size or np.array_equal(got, want) else int(np.flatnonzero(got != want)[0]), "layout": K.layout(origin[:8 * K.KEY_IC].tobytes() + bytes(origin.size - 8 * K.KEY_IC))}
        res["record"] = {"hex": rec.tobytes().hex(), "head": origin[:8 * K.KEY_HEAD_WORDS].tobytes().hex(), "delta1_before": origin[8 * K.KEY_DELTA1:8 * K.KEY_DELTA1 + 64].tobytes().hex()}
        res["contribute_seconds"] = list(sec_c)
        res["chain"] = hip.verify_key_contributions(ctx, origin, got, rec, seconds=sec_v)
        res["chain_seconds"] = list(sec_v)
        res["chain_without_the_record"] = hip.verify_key_contributions(ctx, origin, got, b"")
        spoiled = got.copy()
        where = K.layout(origin[:8 * K.KEY_IC].tobytes() + bytes(origin.size - 8 * K.KEY_IC))
        i, j = where["off_lh"] + 8 * 100000, where["off_lh"] + 8 * 100001
        spoiled[8 * i:8 * i + 64], spoiled[8 * j:8 * j + 64] = got[8 * j:8 * j + 64].copy(), got[8 * i:8 * i + 64].copy()      # two points swapped deep inside l
        res["chain_two_points_swapped"] = hip.verify_key_contributions(ctx, origin, spoiled, rec)
        # a proof under the contributed key
        d2 = hip.Decider.load_key(bench.cf, got)
        try:
            words, pub, _ = d2.prove()
            lz = bench.circuit.len_z
            z0, zi = pub[2:2 + lz], pub[2 + lz:2 + 2 * lz]
            res["proof"] = {"words": [hex(w) for w in words], "steps": STEPS, "z0": [hex(int(x)) for x in z0], "z_i": [hex(int(x)) for x in zi], "verify": d2.verify(STEPS, z0, zi, words),
                            "verify_origin_key": d0.verify(STEPS, z0, zi, words), "key_words": hex_of(d2.key_words()), "info": d2.info()}
        finally:
            d2.close()
        d0.close()
        paths = {x: f"{out_path}.{x}" for x in ("origin.key", "contributed.key", "records", "next.key")}
        origin.tofile(paths["origin.key"]); got.tofile(paths["contributed.key"])
        with open(paths["records"], "wb") as fp:
            fp.write(rec.tobytes())
        res["cli"] = {}
        for name, argv in (("verify", ["verify-contributions", paths["origin.key"], paths["contributed.key"], paths["records"]]),
                           ("contribute", ["contribute", paths["contributed.key"], paths["next.key"], paths["records"]]),
                           ("verify_next", ["verify-contributions", paths["origin.key"], paths["next.key"], paths["records"]]),
                           ("verify_stale_final", ["verify-contributions", paths["origin.key"], paths["contributed.key"], paths["records"]])):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
                rc = iden3._main(argv)
            res["cli"][name] = {"rc": rc, "stdout": buf.getvalue()}
    finally:
        bench.close()
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"key contribution decider probe ok: domain {res['info']['domain']}, keys identical: {res['key']['identical']}, chain {res['chain']}, contribute {[round(x, 3) for x in res['contribute_seconds']]} s, "
          f"verify {[round(x, 3) for x in res['chain_seconds']]} s, {res['seconds']:.1f} s in all")


def main_measure(out_path, full=False):
    """what profiles/key_contrib.txt records: contribute's and verify's stage times (three calls each) and the combination through both forms of the testing hook,
    alternating, `reps` synchronised repetitions a call on the uploaded arrays, over l‖h of the origin and of the contributed key"""
    t_start = time.time()
    from vimz_amd import _lib, hip
    ctx, fixed_mul = open_context()
    bench = DeciderBench(ctx, fixed_mul, "contrast" if full else "hash", light=not full)
    res = {"full": full}
    try:
        d0 = bench.trapdoor_decider(DELTA)
        res["info"] = d0.info()
        origin = d0.save_key()
        d0.close()
        res["contribute_seconds"], res["verify_seconds"] = [], []
        for _ in range(3):
            sec = []
            got, rec = hip.contribute_key(ctx, origin, seconds=sec)
            res["contribute_seconds"].append(list(sec))
        for _ in range(3):
            sec = []
            res["verdict"] = hip.verify_key_contributions(ctx, origin, got, rec, seconds=sec)
            res["verify_seconds"].append(list(sec))
        L = K.layout(origin[:8 * K.KEY_IC].tobytes() + bytes(origin.size - 8 * K.KEY_IC))
        n = L["n_lh"]
        res["n_lh"] = n
        lh = lambda blob: np.ascontiguousarray(blob[8 * L["off_lh"]:8 * (L["off_lh"] + 8 * n)]).view(np.uint64)      # noqa: E731
        b, a = lh(origin), lh(got)
        rho = np.frombuffer(np.random.default_rng(7).bytes(16 * n), dtype="<u8").astype(np.uint64)
        reps = 5
        res["forms"] = {"1": [], "2": []}
        outs = {}
        for rnd in range(4):                                   # (the first round warms both forms up and is kept apart)
            for launches in (1, 2):
                out, secs = np.zeros((2, 8), dtype=np.uint64), np.zeros(reps, dtype=np.float64)
                ctx._chk(ctx.lib.vimz_test_ratio_rlc_forms(ctx.h, hip._ptr(b), hip._ptr(a), n, hip._ptr(rho), _lib.FORM_CANONICAL, launches, reps, hip._ptr(out), hip._ptr(secs)))
                res["forms"][str(launches)].append([float(x) for x in secs])
                outs[launches] = hex_of(out)
        res["forms_agree"] = outs[1] == outs[2]
    finally:
        bench.close()
        ctx.close()
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1] == "measure":
        main_measure(sys.argv[2], full=len(sys.argv) > 3 and sys.argv[3] == "full")
    else:
        {"kernels": main_kernels, "api": main_api, "decider": main_decider}[sys.argv[1]](sys.argv[2])
