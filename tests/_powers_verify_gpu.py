"""GPU half of tests/test_gpu_powers_verify.py, a process of its own per part with VIMZ_HIP_LIBRARY=testing (`python -m tests._powers_verify_gpu
{kernels|api|decider} OUT.json`): judging a powers-of-tau string (vimz_powers_verify; vimz_amd/csrc/g16_powers_verify.hip).

kernels: the two device stages through vimz_test_powers_rlc and vimz_test_powers_flags over the cases of tests/_powers_verify_ref.py, in G1 and in G2.  Points are
[s_i]G made by vimz_test_g16_fixed_mul, the expected sums [Σ rho_i·s_i]G made the same way.
api: vimz_powers_verify over strings of known (tau, alpha, beta) made by the same hook — good ones, and REFUSED's with one thing wrong each —, its bad arguments,
hip.verify_powers and the command line over a `.ptau` container.
decider: the light decider of the hash step over a string of its domain's power: the prefix's verdict and times, hip.Decider and hip.kzg_from_powers with
verify_powers=True over a good string and over one with a wrong point, and the same bad string with the default flag.
Vectors leave as the hex of their little-endian words and nothing is judged here.  Test infrastructure."""
import contextlib
import ctypes as C
import io
import json
import sys
import time

import numpy as np

from tests import _g16_powers_ref as W
from tests import _powers_verify_ref as V
from tests._decider_powers_gpu import ptau_bytes
from tests._g16_kernels_gpu import hex_of, to_words
from tests._pairing import Q, R

TAU, ALPHA, BETA = 0x2545F4914F6CDD1D0123456789ABCDEF, 0xFEDCBA987654321, 0x55AA55AA55AA77
POWER, SMALL_POWER = 5, 3                 # n = 32: tau_g1 has 62 pairs, several chunks of the combination; the issue's string of power 3
N, N_G1 = 1 << POWER, (2 << POWER) - 1
C_, MID = V.RLC_CHUNK, N // 2
N_SRS = 36000
NAMES = ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")


def _ratio_bit(name):
    return {"tau_g1": V.RATIO_TAU_G1, "tau_g2": V.RATIO_TAU_G2, "alpha_g1": V.RATIO_ALPHA_G1, "beta_g1": V.RATIO_BETA_G1}[name]


def refused_cases():
    """name -> (what to change, the verdict's bits, first_bad).  A change is ("scalars", array, {index: scalar}) — valid points of other scalars — or ("points", array,
    {index: kind or point}).  The bits follow from the equations (include/vimz_hip.h): a wrong tau_g1[1] also breaks the halves and the tau_g2 ratio, which is
    measured against it; a wrong tau_g2[1] breaks every ratio measured against it."""
    sc = W.string_scalars(TAU, ALPHA, BETA, POWER)
    cases = {}
    for name in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1"):
        last = len(sc[name]) - 1
        for where, i in (("index_1", 1), ("middle", last // 2), ("last", last)):
            bits = _ratio_bit(name)
            if i == 1 and name == "tau_g1":
                bits |= V.HALVES | V.RATIO_TAU_G2
            if i == 1 and name == "tau_g2":
                bits |= V.HALVES | V.RATIO_TAU_G1 | V.RATIO_ALPHA_G1 | V.RATIO_BETA_G1
            cases[f"wrong_point/{name}/{where}"] = (("scalars", name, {i: (sc[name][i] + 1) % R}), bits, (0, 0))
    c = 0x1234567
    for k in (C_, C_ + 1, N_G1 - 1):      # the broken pair k − 1: the last of chunk 0, the first of chunk 1, the last pair
        cases[f"scaled_from/{k}"] = (("scalars", "tau_g1", {i: c * sc["tau_g1"][i] % R for i in range(k, N_G1)}), V.RATIO_TAU_G1, (0, 0))
    cases["alpha_over_another_tau"] = (("scalars", "alpha_g1", {i: ALPHA * pow(TAU + 1, i, R) % R for i in range(1, N)}), V.RATIO_ALPHA_G1, (0, 0))
    cases["tau_g2_over_another_tau_from_2"] = (("scalars", "tau_g2", {i: pow(TAU + 1, i, R) for i in range(2, N)}), V.RATIO_TAU_G2, (0, 0))
    cases["beta_g2_of_another_beta"] = (("scalars", "beta_g2", {0: BETA + 1}), V.BETA, (0, 0))
    cases["mixed_point_in_tau_g2"] = (("points", "tau_g2", {MID: "mixed"}), V.SUBGROUP, (2, MID))
    cases["beta_g2_outside"] = (("points", "beta_g2", {0: "a"}), V.SUBGROUP, (5, 0))
    cases["tau_g1_0_is_2g"] = (("scalars", "tau_g1", {0: 2}), V.FIRST, (1, 0))
    cases["tau_g2_0_is_2g"] = (("scalars", "tau_g2", {0: 2}), V.FIRST, (2, 0))
    cases["off_curve"] = (("points", "tau_g1", {40: "y_plus_1"}), V.OFF_CURVE, (1, 40))
    cases["coordinate_is_q"] = (("points", "alpha_g1", {7: "x_is_q"}), V.COORD, (3, 7))
    cases["identity"] = (("points", "beta_g1", {N - 1: "identity"}), V.IDENTITY, (4, N - 1))
    return cases


def open_context():
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    vp = C.c_void_p
    ctx.lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    ctx.lib.vimz_test_powers_flags.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, vp]
    ctx.lib.vimz_test_powers_rlc.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, C.c_int, vp]
    ctx.lib.vimz_powers_verify.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(C.c_uint32), vp, C.POINTER(C.c_double)]

    def fixed_mul(group, scalars):
        out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
        ctx._chk(ctx.lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(to_words(scalars)), len(scalars), hip._ptr(out)))
        return out
    return ctx, fixed_mul


def point_words(group, p):
    return to_words(V.flat(group, p)).reshape(-1)


def main_kernels(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    ctx, fixed_mul = open_context()
    cn = _lib.FORM_CANONICAL
    res = {"rlc": {}, "flags": {}}
    try:
        s = V.base_scalars()
        for group in (1, 2):
            base = fixed_mul(group, s)
            cases = V.rlc_cases(group)
            want = []
            for name, rho in cases.items():
                n = len(rho) + 1
                rw = np.frombuffer(b"".join(x.to_bytes(16, "little") for x in rho), dtype="<u8").astype(np.uint64)
                out = np.full((2, 8 * group), 7, dtype=np.uint64)
                t0 = time.time()
                ctx._chk(ctx.lib.vimz_test_powers_rlc(ctx.h, group, hip._ptr(np.ascontiguousarray(base[:n])), n, hip._ptr(rw), cn, hip._ptr(out)))
                res["rlc"][f"{group}/{name}"] = {"out": hex_of(out), "seconds": time.time() - t0}
                want += list(V.rlc_scalars(s, rho))
            pts = fixed_mul(group, want)
            for k, name in enumerate(cases):
                res["rlc"][f"{group}/{name}"]["want"] = hex_of(pts[2 * k:2 * k + 2])
            kinds = V.bad_points(group)
            for name, (sc, bad) in V.flags_cases(group).items():
                arr = fixed_mul(group, sc)
                for i, kind in bad.items():
                    arr[i] = point_words(group, kinds[kind][0])
                flags = np.full(len(sc), 0xDEAD, dtype=np.uint32)
                ctx._chk(ctx.lib.vimz_test_powers_flags(ctx.h, group, hip._ptr(arr), len(sc), cn, hip._ptr(flags)))
                res["flags"][f"{group}/{name}"] = [int(x) for x in flags]
    finally:
        ctx.close()
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"powers verify kernels probe ok: {len(res['rlc'])} combinations, {len(res['flags'])} flag arrays, {res['seconds']:.1f} s")


def verify_raw(ctx, a, n_tau_g1=None, n_pow=None, form=None, null=None):
    from vimz_amd import _lib, hip
    result, first, sec = C.c_uint32(0xFFFF), np.full(2, 7, dtype=np.uint64), (C.c_double * 4)()
    ptr = lambda name: None if null == name else hip._ptr(a[name])      # noqa: E731
    rc = ctx.lib.vimz_powers_verify(ctx.h if null != "ctx" else None, ptr("tau_g1"), a["tau_g1"].shape[0] if n_tau_g1 is None else n_tau_g1, ptr("tau_g2"), ptr("alpha_g1"),
                                    ptr("beta_g1"), a["tau_g2"].shape[0] if n_pow is None else n_pow, ptr("beta_g2"), _lib.FORM_CANONICAL if form is None else form,
                                    None if null == "result" else C.byref(result), None if null == "first_bad" else hip._ptr(first), None if null == "seconds" else sec)
    return {"rc": rc, "result": int(result.value), "first_bad": [int(first[0]), int(first[1])], "seconds": list(sec)}


def string_arrays(fixed_mul, sc):
    return {name: fixed_mul(V.GROUP[name], sc[name]) for name in NAMES}


def main_api(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip, iden3
    ctx, fixed_mul = open_context()
    res = {"refused": {}, "bad_arguments": {}}
    try:
        sc = W.string_scalars(TAU, ALPHA, BETA, POWER)
        good = string_arrays(fixed_mul, sc)
        small = string_arrays(fixed_mul, W.string_scalars(TAU, ALPHA, BETA, SMALL_POWER))
        res["accepted"] = {"power_3": verify_raw(ctx, small), "power_5": verify_raw(ctx, good), "prefix": verify_raw(ctx, good, n_tau_g1=15, n_pow=8),
                           "prefix_without_2n_minus_1": verify_raw(ctx, good, n_tau_g1=N, n_pow=N)}
        kinds = {group: V.bad_points(group) for group in (1, 2)}
        for name, (change, _bits, _first) in refused_cases().items():
            how, array, at = change
            a = dict(good)
            if how == "scalars":
                s = list(sc[array])
                for i, x in at.items():
                    s[i] = x
                a[array] = fixed_mul(V.GROUP[array], s)
            else:
                a[array] = good[array].copy()
                for i, kind in at.items():
                    a[array][i] = point_words(V.GROUP[array], kinds[V.GROUP[array]][kind][0])
            res["refused"][name] = verify_raw(ctx, a)
        # two arrays with a finding each: the first ARRAY's is reported, whatever the order they were looked at in
        two = dict(good, beta_g1=good["beta_g1"].copy(), tau_g2=good["tau_g2"].copy())
        two["beta_g1"][3] = point_words(1, kinds[1]["y_plus_1"][0]); two["tau_g2"][5] = 0
        res["two_findings"] = verify_raw(ctx, two)
        # a wrong point beyond the prefix that is judged is not looked at
        beyond = dict(good, tau_g1=good["tau_g1"].copy())
        beyond["tau_g1"][40] = point_words(1, kinds[1]["y_plus_1"][0])
        res["beyond_the_prefix"] = verify_raw(ctx, beyond, n_tau_g1=15, n_pow=8)
        res["bad_arguments"] = {f"null_{x}": verify_raw(ctx, good, null=x)["rc"] for x in ("ctx", "tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2", "result", "first_bad")}
        res["bad_arguments"].update({"n_pow_1": verify_raw(ctx, good, n_pow=1)["rc"], "n_tau_g1_below_n_pow": verify_raw(ctx, good, n_tau_g1=N - 1)["rc"],
                                     "form_7": verify_raw(ctx, good, form=7)["rc"]})
        res["null_seconds"] = verify_raw(ctx, good, null="seconds")
        # the Python call and the command line over a .ptau container (the file's Montgomery form)
        ptau = ptau_bytes(POWER, good)
        powers = iden3.read_ptau(ptau)
        sec = []
        res["python"] = {"whole": hip.verify_powers(ctx, powers, seconds=sec), "seconds": list(sec), "n_8": hip.verify_powers(ctx, powers, 8)}
        bad_ptau = ptau_bytes(POWER, dict(good, tau_g2=res_point(good["tau_g2"], MID, point_words(2, kinds[2]["mixed"][0]))))
        bad = iden3.read_ptau(bad_ptau)
        res["python"]["mixed"] = hip.verify_powers(ctx, bad)
        res["python"]["mixed_beyond_n_8"] = hip.verify_powers(ctx, bad, 8)
        refusals = {}
        for name, fn in (("n_1", lambda: hip.verify_powers(ctx, powers, 1)), ("n_above", lambda: hip.verify_powers(ctx, powers, N + 1))):
            try:
                fn(); refusals[name] = 0
            except _lib.VimzError as e:
                refusals[name] = e.code
        res["python"]["refusals"] = refusals
        good_path, bad_path = out_path + ".good.ptau", out_path + ".bad.ptau"
        with open(good_path, "wb") as fp:
            fp.write(ptau)
        with open(bad_path, "wb") as fp:
            fp.write(bad_ptau)
        res["cli"] = {}
        for name, argv in (("good", ["verify", good_path]), ("good_8", ["verify", good_path, "8"]), ("bad", ["verify", bad_path]), ("usage", ["verify"])):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
                rc = iden3._main(argv)
            res["cli"][name] = {"rc": rc, "stdout": buf.getvalue()}
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"powers verify api probe ok: {len(res['refused'])} refused strings, {res['seconds']:.1f} s")


def res_point(array, index, words):
    a = array.copy()
    a[index] = words
    return a


def main_decider(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip, iden3
    from vimz_amd.circuit import Circuit
    ctx, fixed_mul = open_context()
    res = {}
    c = Circuit.for_resolution("hash", "HD")
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
    srs = cf = None
    try:
        power = 18                                             # the light hash decider's domain (asserted below from the decider itself)
        sc = W.string_scalars(TAU, ALPHA, BETA, power)
        canon = string_arrays(fixed_mul, sc)
        powers = iden3.read_ptau(ptau_bytes(power, canon))
        srs, _vk = hip.kzg_from_powers(ctx, powers, N_SRS)
        cf = hip.CycleFoldIVC(ctx, c, srs, ck2, max_batch=2)

        def attempt(fn):
            t0 = time.time()
            try:
                d = fn()
            except _lib.VimzError as e:
                return {"code": e.code, "message": str(e), "seconds": time.time() - t0}
            out = {"code": 0, "seconds": time.time() - t0}
            if isinstance(d, hip.Decider):
                out["info"], out["setup_seconds"] = d.info(), d.setup_seconds
                d.close()
            else:
                d[0].free()
            return out
        res["good_verified"] = attempt(lambda: hip.Decider(cf, powers=powers, light=True, verify_powers=True))
        n = res["good_verified"]["info"]["domain"]
        res["domain"] = n
        sec = []
        hip.verify_powers(ctx, powers, n)                      # (the first call of a process pays for the kernels' load)
        res["verdict"] = hip.verify_powers(ctx, powers, n, seconds=sec)
        res["verdict_seconds"] = list(sec)
        # one wrong point — a valid point of G1, so the set-up's own checks pass it — deep inside the prefix
        where = 1000
        bad = dict(powers, tau_g1=np.array(powers["tau_g1"]))
        bad["tau_g1"][where] = powers["tau_g1"][where + 1]
        res["bad_verdict"] = hip.verify_powers(ctx, bad, n)
        res["bad_verified"] = attempt(lambda: hip.Decider(cf, powers=bad, light=True, verify_powers=True))
        res["bad_default"] = attempt(lambda: hip.Decider(cf, powers=bad, light=True))
        res["kzg_bad_verified"] = attempt(lambda: hip.kzg_from_powers(ctx, bad, N_SRS, verify_powers=True))
        res["kzg_bad_default"] = attempt(lambda: hip.kzg_from_powers(ctx, bad, N_SRS))
        res["flag_without_powers"] = attempt(lambda: hip.Decider(cf, light=True, verify_powers=True))
    finally:
        if cf is not None:
            cf.close()
        if srs is not None:
            srs.free()
        ck2.free()
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"powers verify decider probe ok: domain {res['domain']}, verdict {res['verdict']}, seconds {[round(x, 3) for x in res['verdict_seconds']]}, {res['seconds']:.1f} s in all")


if __name__ == "__main__":
    {"kernels": main_kernels, "api": main_api, "decider": main_decider}[sys.argv[1]](sys.argv[2])
