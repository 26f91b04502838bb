"""GPU half of tests/test_gpu_powers_contrib.py, a process of its own per part with VIMZ_HIP_LIBRARY=testing (`python -m tests._powers_contrib_gpu {kernels|api|decider}
OUT.json`): a contribution to a powers-of-tau string and the check of a chain of them (vimz_powers_contribute, vimz_powers_verify_contributions; vimz_amd/csrc/
g16_powers_contrib.hip).

kernels: k_power_vec through vimz_test_power_vec over tests/_powers_contrib_ref.POWER_COUNTS x POWER_WS, and k_scale_points_by through vimz_test_scale_points_by over
scale_cases() in G1 and G2.  Points are [s_i]G made by vimz_test_g16_fixed_mul, the expected outputs [c·w^i·s_i]G made the same way.
api: the two calls on strings of known scalars — contribute with fixed secrets and nonces beside the reference's string and record (also with the outputs on the
inputs, and on a prefix), the result through vimz_powers_verify, chains of 0, 1 and 3 records, a chain from iden3.new_powers, every tampered chain, contribute's
refusals, bad arguments, the production entry (secrets from the OS), hip's wrappers and the three commands of `python -m vimz_amd.iden3`.
decider: once, on the light decider of the hash step (domain 2^18): a string made as tests/_decider_powers_gpu.py makes it, contributed to through the production
entry, the chain's verdict, then hip.kzg_from_powers, hip.Decider(powers=) and a proof under that key.
Vectors leave as hex and nothing is judged here.  Test infrastructure."""
import contextlib
import ctypes as C
import io
import json
import sys
import time

import numpy as np

from tests import _powers_contrib_ref as K
from tests import _powers_verify_ref as V
from tests._g16_kernels_gpu import from_words, hex_of, to_words
from tests._pairing import Q, R

NAMES = ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")
TAU, ALPHA, BETA = 0x2545F4914F6CDD1D0123456789ABCDEF, 0xFEDCBA987654321, 0x55AA55AA55AA77      # the end-to-end string's, as tests/_decider_powers_gpu.py's
N_SRS, STEPS = 36000, 4


def open_context():
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    vp, st = C.c_void_p, C.c_size_t
    ctx.lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, st, vp]
    ctx.lib.vimz_test_power_vec.argtypes = [vp, vp, st, vp]
    ctx.lib.vimz_test_scale_points_by.argtypes = [vp, C.c_int, vp, st, vp, vp, C.c_int, vp]
    contribute = [vp, vp, st, vp, vp, vp, st, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    ctx.lib.vimz_powers_contribute.argtypes = contribute + [C.POINTER(C.c_double)]
    ctx.lib.vimz_testing_powers_contribute_secrets.argtypes = contribute + [vp, vp, C.POINTER(C.c_double)]
    ctx.lib.vimz_powers_verify_contributions.argtypes = [vp, vp, vp, st, vp, vp, vp, st, vp, C.c_int, vp, st, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, C.POINTER(C.c_double)]
    ctx.lib.vimz_powers_verify.argtypes = [vp, vp, st, vp, vp, vp, st, vp, C.c_int, C.POINTER(C.c_uint32), vp, C.POINTER(C.c_double)]

    def fixed_mul(group, scalars):
        out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
        ctx._chk(ctx.lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(to_words(scalars)), len(scalars), hip._ptr(out)))
        return out
    return ctx, fixed_mul


def mont(arr):
    """canonical coordinates -> the Montgomery form, same shape"""
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return np.frombuffer(b"".join((x * (1 << 256) % Q).to_bytes(32, "little") for x in from_words(a)), dtype="<u8").astype(np.uint64).reshape(a.shape)


def main_kernels(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    ctx, fixed_mul = open_context()
    res = {"power": {}, "scale": {"1": {}, "2": {}}}
    try:
        for count in K.POWER_COUNTS:
            for name, w in K.POWER_WS.items():
                out = np.full((count, 4), 7, dtype=np.uint64)
                ctx._chk(ctx.lib.vimz_test_power_vec(ctx.h, hip._ptr(to_words([w])), count, hip._ptr(out)))
                res["power"][f"{count}/{name}"] = hex_of(out)
        for group in (1, 2):
            for name, (s, w, c, form, in_place) in K.scale_cases(group).items():
                n = len(s)
                pts, want = fixed_mul(group, s), fixed_mul(group, K.scale_expected(s, w, c))
                if form == "montgomery":
                    pts, want = mont(pts), mont(want)
                before = pts.copy()
                out = pts if in_place else np.full((n, 8 * group), 7, dtype=np.uint64)
                ctx._chk(ctx.lib.vimz_test_scale_points_by(ctx.h, group, hip._ptr(pts), n, hip._ptr(to_words([w])), hip._ptr(to_words([c])),
                                                           _lib.FORM_MONTGOMERY if form == "montgomery" else _lib.FORM_CANONICAL, hip._ptr(out)))
                res["scale"][str(group)][name] = {"out": hex_of(out), "want": hex_of(want), "input": hex_of(before), "input_kept": in_place or bool(np.array_equal(pts, before))}
        pts, out, one = fixed_mul(1, K.scale_inputs(9)), np.zeros((9, 8), dtype=np.uint64), to_words([1])
        off = pts.copy(); off[3, 4] ^= np.uint64(1)
        call = lambda group, p, n, w, c, form, o: ctx.lib.vimz_test_scale_points_by(ctx.h, group, p, n, w, c, form, o)      # noqa: E731
        res["bad_arguments"] = {"n_0": call(1, hip._ptr(pts), 0, hip._ptr(one), hip._ptr(one), 0, hip._ptr(out)), "group_3": call(3, hip._ptr(pts), 9, hip._ptr(one), hip._ptr(one), 0, hip._ptr(out)),
                                "form_7": call(1, hip._ptr(pts), 9, hip._ptr(one), hip._ptr(one), 7, hip._ptr(out)), "null_out": call(1, hip._ptr(pts), 9, hip._ptr(one), hip._ptr(one), 0, None),
                                "w_is_r": call(1, hip._ptr(pts), 9, hip._ptr(to_words([R])), hip._ptr(one), 0, hip._ptr(out)), "off_curve": call(1, hip._ptr(off), 9, hip._ptr(one), hip._ptr(one), 0, hip._ptr(out)),
                                "power_count_0": ctx.lib.vimz_test_power_vec(ctx.h, hip._ptr(one), 0, hip._ptr(out)), "power_w_is_r": ctx.lib.vimz_test_power_vec(ctx.h, hip._ptr(to_words([R])), 2, hip._ptr(out))}
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"powers contribution kernels probe ok: {len(res['power'])} power vectors, {len(res['scale']['1'])} + {len(res['scale']['2'])} scalings, {res['seconds']:.1f} s")


# ---- the two calls themselves --------------------------------------------------------------------------------------------------------------------------
def string_arrays(fixed_mul, scalars):
    """a string of scalars -> canonical uint64 rows, the points made by the fixed-base hook"""
    return {name: fixed_mul(V.GROUP[name], scalars[name]) for name in NAMES}


def points_arrays(string):
    """a string of Python points (coordinates possibly not below q) -> canonical uint64 rows"""
    return {name: np.frombuffer(b"".join(c.to_bytes(32, "little") for p in string[name] for c in V.flat(V.GROUP[name], p)), dtype="<u8").astype(np.uint64).reshape(len(string[name]), -1)
            for name in NAMES}


def origin_words(points):
    return np.frombuffer(K.points_bytes(points), dtype="<u8").astype(np.uint64)


def contribute_raw(ctx, arrays, secrets=None, nonces=None, in_place=False, null=None, n_tau_g1=None, n_pow=None, form=0):
    """the C call itself: {"rc", "out" (name -> hex), "record" (hex), "seconds", "message"}"""
    from vimz_amd import hip
    src = {name: np.ascontiguousarray(arrays[name], dtype=np.uint64).copy() for name in NAMES}
    dst = src if in_place else {name: np.full(src[name].shape, 0xEE, dtype=np.uint64) for name in NAMES}
    rec, sec = np.full(61, 7, dtype=np.uint64), (C.c_double * 3)()
    ptr = lambda d, name, tag: None if null == tag + name else hip._ptr(d[name])      # noqa: E731
    args = [None if null == "ctx" else ctx.h, ptr(src, "tau_g1", ""), src["tau_g1"].shape[0] if n_tau_g1 is None else n_tau_g1, ptr(src, "tau_g2", ""), ptr(src, "alpha_g1", ""),
            ptr(src, "beta_g1", ""), src["tau_g2"].shape[0] if n_pow is None else n_pow, ptr(src, "beta_g2", ""), form] + [ptr(dst, name, "out_") for name in NAMES] + \
           [None if null == "record" else hip._ptr(rec)]
    if secrets is None:
        rc = ctx.lib.vimz_powers_contribute(*args, None if null == "seconds" else sec)
    else:
        rc = ctx.lib.vimz_testing_powers_contribute_secrets(*args, None if null == "secrets" else hip._ptr(to_words(secrets)), hip._ptr(to_words(nonces)), sec)
    return {"rc": int(rc), "out": {name: hex_of(dst[name]) for name in NAMES}, "record": rec.tobytes().hex(), "seconds": list(sec),
            "untouched": not in_place and all(bool((dst[name] == 0xEE).all()) for name in NAMES) and bool((rec == 7).all()),
            "message": ctx.lib.vimz_last_error(ctx.h).decode() if rc and null != "ctx" else ""}


def verify_raw(ctx, origin, arrays, records, null=None, n_records=None, n_pow=None, form=0):
    from vimz_amd import hip
    a = {name: np.ascontiguousarray(arrays[name], dtype=np.uint64) for name in NAMES}
    o, r = np.ascontiguousarray(origin, dtype=np.uint64), np.frombuffer(bytes(records), dtype=np.uint8).copy()
    result, sresult, first, sec = C.c_uint32(0xFFFF), C.c_uint32(0xFFFF), np.full(2, 7, dtype=np.uint64), (C.c_double * 3)()
    ptr = lambda name: None if null == name else hip._ptr(a[name])      # noqa: E731
    rc = ctx.lib.vimz_powers_verify_contributions(None if null == "ctx" else ctx.h, None if null == "origin" else hip._ptr(o), ptr("tau_g1"), a["tau_g1"].shape[0], ptr("tau_g2"), ptr("alpha_g1"),
                                                  ptr("beta_g1"), a["tau_g2"].shape[0] if n_pow is None else n_pow, ptr("beta_g2"), form, hip._ptr(r) if r.size and null != "records" else None,
                                                  r.size // K.RECORD_BYTES if n_records is None else n_records, None if null == "result" else C.byref(result),
                                                  None if null == "string_result" else C.byref(sresult), None if null == "first_bad" else hip._ptr(first), None if null == "seconds" else sec)
    return {"rc": rc, "result": int(result.value), "string_result": int(sresult.value), "first_bad": [int(first[0]), int(first[1])], "seconds": list(sec),
            "message": ctx.lib.vimz_last_error(ctx.h).decode() if rc and null != "ctx" else ""}


def powers_verify_raw(ctx, a, form=0):
    from vimz_amd import hip
    result, first = C.c_uint32(0xFFFF), np.full(2, 7, dtype=np.uint64)
    rc = ctx.lib.vimz_powers_verify(ctx.h, hip._ptr(a["tau_g1"]), a["tau_g1"].shape[0], hip._ptr(a["tau_g2"]), hip._ptr(a["alpha_g1"]), hip._ptr(a["beta_g1"]), a["tau_g2"].shape[0],
                                    hip._ptr(a["beta_g2"]), form, C.byref(result), hip._ptr(first), None)
    return [rc, int(result.value), [int(first[0]), int(first[1])]]


def unhex(out, like):
    return {name: np.frombuffer(bytes.fromhex(out[name]), dtype="<u8").astype(np.uint64).reshape(like[name].shape) for name in NAMES}


def run_cli(argv):
    from vimz_amd import iden3
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        rc = iden3._main(argv)
    return {"rc": rc, "stdout": buf.getvalue()}


def main_api(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip, iden3
    ctx, fixed_mul = open_context()
    res = {}
    try:
        # contribute beside the reference, word for word; the result through vimz_powers_verify
        res["contribute"] = {}
        want_rec = K.chain_records(1).hex()
        for power in K.POWERS:
            before, after = (string_arrays(fixed_mul, s) for s in K.chain_scalars(power, 1))
            want = {name: hex_of(after[name]) for name in NAMES}
            got = contribute_raw(ctx, before, K.SECRET_SETS[0], K.NONCE_SETS[0])
            same = contribute_raw(ctx, before, K.SECRET_SETS[0], K.NONCE_SETS[0], in_place=True)
            res["contribute"][str(power)] = {"rc": got["rc"], "points": got["out"] == want, "record": got["record"] == want_rec, "in_place_rc": same["rc"], "in_place_points": same["out"] == want,
                                             "in_place_record": same["record"] == want_rec, "seconds": got["seconds"], "n_tau_g1": int(before["tau_g1"].shape[0]),
                                             "powers_verify": powers_verify_raw(ctx, unhex(got["out"], before)), "differs": got["out"]["tau_g1"] != hex_of(before["tau_g1"])}
            if power == 1:
                res["spot"] = {"out": got["out"], "record": got["record"]}
        before, after = (string_arrays(fixed_mul, s) for s in K.chain_scalars(3, 1))
        cut = lambda a: {name: a[name][:8] if name != "beta_g2" else a[name] for name in NAMES}      # noqa: E731
        got = contribute_raw(ctx, cut(before), K.SECRET_SETS[0], K.NONCE_SETS[0])
        res["prefix"] = {"rc": got["rc"], "points": got["out"] == {name: hex_of(cut(after)[name]) for name in NAMES}, "record": got["record"] == want_rec}
        m = contribute_raw(ctx, {name: mont(before[name]) for name in NAMES}, K.SECRET_SETS[0], K.NONCE_SETS[0], form=_lib.FORM_MONTGOMERY)
        res["montgomery"] = {"rc": m["rc"], "points": m["out"] == {name: hex_of(mont(after[name])) for name in NAMES}, "record": m["record"] == want_rec}
        # the chains
        res["accepted"] = {}
        for power, n in ((K.TAMPER_POWER, 0), (K.TAMPER_POWER, 1), (K.TAMPER_POWER, 3), (7, 3)):
            strings = K.chain_scalars(power, n)
            res["accepted"][f"{power}/{n}"] = verify_raw(ctx, origin_words(K.scalar_points(K.triple(strings[0]))), string_arrays(fixed_mul, strings[-1]), K.chain_records(n))
        strings = K.chain_scalars(K.TAMPER_POWER, 1)
        final1 = string_arrays(fixed_mul, strings[-1])
        res["accepted"]["null_seconds"] = verify_raw(ctx, origin_words(K.scalar_points(K.triple(strings[0]))), final1, K.chain_records(1), null="seconds")
        res["accepted"]["montgomery"] = verify_raw(ctx, origin_words(K.scalar_points(K.triple(strings[0]))), {name: mont(final1[name]) for name in NAMES}, K.chain_records(1), form=_lib.FORM_MONTGOMERY)
        # from the new string: the hook beside the reference, and a chain of two production contributions
        new = iden3.new_powers(1)
        k1, r1 = hip.contribute_powers(ctx, new, secrets=K.SECRET_SETS[0], nonces=K.NONCE_SETS[0])
        want = string_arrays(fixed_mul, K.chain_scalars(1, 1, new=True)[1])
        new2 = iden3.new_powers(2)
        a, ra = hip.contribute_powers(ctx, new2)
        b, rb = hip.contribute_powers(ctx, a)
        res["new"] = {"points": all(hex_of(k1[name]) == hex_of(mont(want[name])) for name in NAMES), "record": r1 == K.chain_records(1, new=True),
                      "chain": hip.verify_powers_contributions(ctx, new2, b, ra + rb), "first_alone": hip.verify_powers_contributions(ctx, new2, a, ra),
                      "no_records": hip.verify_powers_contributions(ctx, new2, new2, b""), "second_without_first": hip.verify_powers_contributions(ctx, new2, b, rb),
                      "powers_verify": hip.verify_powers(ctx, b)}
        # every tampered chain
        res["tampered"] = {name: verify_raw(ctx, origin_words(o), points_arrays(f), r) for name, (o, f, r) in K.tampered_chains().items()}
        # the refusals of contribute, each with its message
        res["refused"] = {name: contribute_raw(ctx, points_arrays(s), K.SECRET_SETS[0], K.NONCE_SETS[0]) for name, s in K.refused_strings().items()}
        for r in res["refused"].values():
            del r["out"], r["record"]
        res["refused_product_entry"] = contribute_raw(ctx, points_arrays(K.refused_strings()["coordinate_is_q"]))["rc"]
        # bad arguments
        s0 = string_arrays(fixed_mul, K.chain_scalars(K.TAMPER_POWER, 0)[0])
        sec, non = K.SECRET_SETS[0], K.NONCE_SETS[0]
        bad = {f"contribute_null_{x}": contribute_raw(ctx, s0, sec, non, null=x)["rc"] for x in ("ctx", "record", "secrets") + NAMES + tuple("out_" + n for n in NAMES)}
        bad.update({"contribute_n_pow_1": contribute_raw(ctx, s0, sec, non, n_pow=1)["rc"], "contribute_short_tau_g1": contribute_raw(ctx, s0, sec, non, n_tau_g1=3)["rc"],
                    "contribute_form_7": contribute_raw(ctx, s0, sec, non, form=7)["rc"], "secret_zero": contribute_raw(ctx, s0, (5, 0, 7), non)["rc"],
                    "secret_is_r": contribute_raw(ctx, s0, (R, 5, 7), non)["rc"], "nonce_is_r": contribute_raw(ctx, s0, sec, (1, 2, R))["rc"]})
        origin, final, records = K.chain()
        ow, fa = origin_words(origin), points_arrays(final)
        bad.update({f"verify_null_{x}": verify_raw(ctx, ow, fa, records, null=x)["rc"] for x in ("ctx", "origin", "records", "result", "string_result", "first_bad") + NAMES})
        bad.update({"verify_record_magic": verify_raw(ctx, ow, fa, K.put(records, K.RECORD_WORDS, b"VG16CTR1"))["rc"], "verify_n_pow_1": verify_raw(ctx, ow, fa, records, n_pow=1)["rc"],
                    "verify_form_7": verify_raw(ctx, ow, fa, records, form=7)["rc"]})
        res["bad_arguments"] = bad
        res["bad_messages"] = {"record_magic": verify_raw(ctx, ow, fa, K.put(records, K.RECORD_WORDS, b"VG16CTR1"))["message"], "n_pow_1": contribute_raw(ctx, s0, sec, non, n_pow=1)["message"]}
        # the production entry: secrets from the OS, twice on the same string
        x, y = contribute_raw(ctx, s0), contribute_raw(ctx, s0)
        xa = unhex(x["out"], s0)
        z = contribute_raw(ctx, xa)
        o0 = origin_words(K.scalar_points(K.triple(K.chain_scalars(K.TAMPER_POWER, 0)[0])))
        res["os_secrets"] = {"rc": [x["rc"], y["rc"], z["rc"]], "strings_differ": all(x["out"][n] != y["out"][n] and x["out"][n] != hex_of(s0[n]) for n in NAMES if n != "tau_g1")
                             and x["out"]["tau_g1"][128:] != y["out"]["tau_g1"][128:], "generators_kept": x["out"]["tau_g1"][:128] == hex_of(s0["tau_g1"][:1]) and x["out"]["tau_g2"][:256] == hex_of(s0["tau_g2"][:1]),
                             "records_differ": x["record"] != y["record"], "chain": verify_raw(ctx, o0, unhex(z["out"], s0), bytes.fromhex(x["record"] + z["record"])),
                             "first_alone": verify_raw(ctx, o0, xa, bytes.fromhex(x["record"])), "other_first": verify_raw(ctx, o0, unhex(z["out"], s0), bytes.fromhex(y["record"] + z["record"]))}
        # hip's wrappers on a dictionary in the file's form, and the command line
        p0 = {name: mont(s0[name]) for name in NAMES}
        p0["power"] = K.TAMPER_POWER
        secs, vsecs = [], []
        k1, r1 = hip.contribute_powers(ctx, p0, secrets=sec, nonces=non, seconds=secs)
        want1 = string_arrays(fixed_mul, K.chain_scalars(K.TAMPER_POWER, 1)[1])
        tam = K.tampered_chains()["record_z/alpha"]
        res["python"] = {"points": all(hex_of(k1[n]) == hex_of(mont(want1[n])) for n in NAMES), "record": r1 == K.chain_records(1), "power": k1["power"], "seconds": list(secs),
                         "verify": hip.verify_powers_contributions(ctx, p0, k1, r1, seconds=vsecs), "verify_seconds": list(vsecs),
                         "verify_points": hip.verify_powers_contributions(ctx, K.scalar_points(K.triple(K.chain_scalars(K.TAMPER_POWER, 0)[0])), k1, r1),
                         "verify_words": hip.verify_powers_contributions(ctx, o0, k1, np.frombuffer(r1, dtype=np.uint8)),
                         "tampered": hip.verify_powers_contributions(ctx, tam[0], {n: mont(v) for n, v in points_arrays(tam[1]).items()}, tam[2]),
                         "problems": hip.powchain_problems(K.LAST | K.STRING), "round_trip": iden3.write_ptau(iden3.read_ptau(iden3.write_ptau(k1))) == iden3.write_ptau(k1)}
        refusals = {}
        for name, fn in (("secrets_without_nonces", lambda: hip.contribute_powers(ctx, p0, secrets=sec)), ("records_length", lambda: hip.verify_powers_contributions(ctx, p0, k1, r1[:-1])),
                         ("one_point_strings", lambda: hip.contribute_powers(ctx, {n: v[:1] for n, v in p0.items() if n != "power"})),
                         ("origin_of_two_points", lambda: hip.verify_powers_contributions(ctx, [(1, 2), (1, 2)], k1, r1)),
                         ("off_curve", lambda: hip.contribute_powers(ctx, {n: mont(v) for n, v in points_arrays(K.refused_strings()["alpha_g1_off_curve"]).items()}))):
            try:
                fn(); refusals[name] = [0, ""]
            except _lib.VimzError as e:
                refusals[name] = [e.code, str(e)]
        res["python"]["refusals"] = refusals
        paths = {x: f"{out_path}.{x}" for x in ("origin.ptau", "one.ptau", "two.ptau", "records")}
        res["cli"] = {"new": run_cli(["new-powers", "2", paths["origin.ptau"]]), "contribute_1": run_cli(["contribute-powers", paths["origin.ptau"], paths["one.ptau"], paths["records"]]),
                      "contribute_2": run_cli(["contribute-powers", paths["one.ptau"], paths["two.ptau"], paths["records"]]),
                      "verify_2": run_cli(["verify-powers-contributions", paths["origin.ptau"], paths["two.ptau"], paths["records"]]),
                      "verify_wrong_final": run_cli(["verify-powers-contributions", paths["origin.ptau"], paths["one.ptau"], paths["records"]]),
                      "usage_new": run_cli(["new-powers", "0", paths["origin.ptau"]]), "usage_contribute": run_cli(["contribute-powers", paths["origin.ptau"]]),
                      "usage_verify": run_cli(["verify-powers-contributions"])}
        with open(paths["records"], "rb") as fp:
            res["cli"]["records_bytes"] = len(fp.read())
        with open(paths["origin.ptau"], "rb") as fp:
            res["cli"]["origin_is_new_powers"] = fp.read() == iden3.write_ptau(iden3.new_powers(2))
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"powers contribution api probe ok: {len(res['tampered'])} tampered chains, {res['seconds']:.1f} s")


def main_decider(out_path):
    t_start = time.time()
    from tests import _g16_powers_ref as W
    from tests._decider_powers_gpu import ptau_bytes
    from tests.test_circuits import step_inputs
    from vimz_amd import _lib, hip, iden3
    from vimz_amd.circuit import Circuit
    ctx, fixed_mul = open_context()
    res = {}
    circuit = Circuit.for_resolution("hash", "HD")
    z0, inputs = step_inputs("hash")
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
    srs = cf = dec = None
    try:
        power = 18                                             # the light hash decider's domain (the test asserts it)
        sc = W.string_scalars(TAU, ALPHA, BETA, power)
        origin = iden3.read_ptau(ptau_bytes(power, {name: fixed_mul(V.GROUP[name], sc[name]) for name in NAMES}))
        sec_c, sec_v = [], []
        powers, rec = hip.contribute_powers(ctx, origin, seconds=sec_c)                                # 1. the production entry
        res["contribute_seconds"], res["record_bytes"] = list(sec_c), len(rec)
        res["string_changed"] = not np.array_equal(powers["tau_g1"][1], origin["tau_g1"][1]) and np.array_equal(powers["tau_g1"][0], origin["tau_g1"][0])
        res["chain"] = hip.verify_powers_contributions(ctx, origin, powers, rec, seconds=sec_v)         # 2. the chain
        res["chain_seconds"] = list(sec_v)
        res["chain_without_the_record"] = hip.verify_powers_contributions(ctx, origin, powers, b"")
        powers = iden3.read_ptau(iden3.write_ptau(powers))                                             # (through the container, as a user's file goes)
        srs, kzg_vk = hip.kzg_from_powers(ctx, powers, N_SRS)                                          # 3. the SRS of the contributed string
        cf = hip.CycleFoldIVC(ctx, circuit, srs, ck2, max_batch=2)
        cf.reset(z0); cf.fold(np.stack(inputs[:STEPS]))
        dec = hip.Decider(cf, powers=powers, light=True)                                               # 4. the key from the contributed string
        res["info"] = dec.info()
        words, pub, _ = dec.prove()                                                                    # 5. a proof under it
        lz = circuit.len_z
        pz0, pzi = pub[2:2 + lz], pub[2 + lz:2 + 2 * lz]
        res["proof"] = {"words": [hex(w) for w in words], "steps": STEPS, "z0": [hex(int(x)) for x in pz0], "z_i": [hex(int(x)) for x in pzi], "verify": dec.verify(STEPS, pz0, pzi, words),
                        "key_words": hex_of(dec.key_words()), "kzg_vk_is_the_contributed_strings": hex_of(mont(kzg_vk)) == hex_of(powers["tau_g2"][1]),
                        "kzg_vk_is_not_the_origins": hex_of(mont(kzg_vk)) != hex_of(origin["tau_g2"][1])}
    finally:
        if dec is not None:
            dec.close()
        if cf is not None:
            cf.close()
        if srs is not None:
            srs.free()
        ck2.free()
        ctx.close()
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"powers contribution decider probe ok: domain {res['info']['domain']}, chain {res['chain']}, contribute {[round(x, 3) for x in res['contribute_seconds']]} s, "
          f"verify {[round(x, 3) for x in res['chain_seconds']]} s, {res['seconds']:.1f} s in all")


if __name__ == "__main__":
    {"kernels": main_kernels, "api": main_api, "decider": main_decider}[sys.argv[1]](sys.argv[2])
