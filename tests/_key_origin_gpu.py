"""GPU half of tests/test_gpu_key_origin.py, a process of its own per part with VIMZ_HIP_LIBRARY=testing (`python -m tests._key_origin_gpu {kernels|driver|decider}
OUT.json`): judging that a decider key derives from a powers-of-tau string and the circuit (vimz_decider_key_verify_origin; vimz_amd/csrc/g16_key_origin.hip).

kernels: k_spmv3_dict through vimz_test_g16_spmv_dict over tests/_key_origin_ref.spmv_cases(), and the hook's refusals of a matrix whose indices are out of bounds.
driver: vimz_test_key_origin — the product's driver on synthetic circuits — over DRIVER_SHAPES: the derived key (points [s]G made by vimz_test_g16_fixed_mul from
derive_key's scalars, the blob assembled here, rho given), the key after one contribution, every tamper of the reference at TAMPER_SHAPE, and the refusals.
decider: once, on the light decider of the hash step (domain 2^18): the key vimz_decider_setup_from_powers saves, the same after contribute_key, a trapdoor key of
another alpha, poked l and b2 points, the other mode, and verify_powers=True on a bad string.
measure (not run by the tests; what profiles/key_origin.txt records): the call's stage times beside the set-up's from the same string, alternating.
Vectors leave as hex and nothing is judged here.  Test infrastructure."""
import contextlib
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

from tests import _key_contrib_ref as K
from tests import _key_origin_ref as O
from tests._g16_kernels_gpu import hex_of, to_words


def open_context():
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    vp = C.c_void_p
    ctx.lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    ctx.lib.vimz_test_g16_spmv_dict.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, vp, vp]
    ctx.lib.vimz_test_key_origin.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_int, vp,
                                             C.POINTER(C.c_uint32), vp, vp]

    def fixed_mul(group, scalars):
        out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
        ctx._chk(ctx.lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(to_words(scalars)), len(scalars), hip._ptr(out)))
        return out
    return ctx, fixed_mul


class Csr:
    """a circuit's three CSRs as the hooks take them: nine pointers and the entry counts (the arrays are kept alive here)"""

    def __init__(self, mats):
        self.arrays = [np.ascontiguousarray(M[k], dtype=np.uint32) for k in range(3) for M in mats]      # row_ptr of A, B, C; col ...; coef ...
        self.ptrs = (C.c_void_p * 9)(*[a.ctypes.data if a.size else None for a in self.arrays])
        self.nnz = (C.c_size_t * 3)(*[len(M[1]) for M in mats])


def main_kernels(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    ctx, _fixed_mul = open_context()
    res = {"spmv": {}, "refused": {}}
    try:
        def run(case, mats=None):
            csr = Csr(mats or case["mats"])
            outs = [np.full((case["n"], 4), 7, dtype=np.uint64) for _ in range(3)]
            t0 = time.time()
            rc = ctx.lib.vimz_test_g16_spmv_dict(ctx.h, csr.ptrs, csr.nnz, hip._ptr(to_words(case["dict"])), len(case["dict"]), case["m"], case["n_c"], case["n"], hip._ptr(to_words(case["v"])),
                                                 *[hip._ptr(o) for o in outs])
            return rc, outs, time.time() - t0
        cases = O.spmv_cases()
        for name, case in cases.items():
            rc, outs, sec = run(case)
            res["spmv"][name] = {"rc": rc, "out": [hex_of(o) for o in outs], "seconds": sec}
        case = cases["63/loose"]
        row_ptr, col, coef = case["mats"][0]
        bad = {"column_is_m": (row_ptr, [case["m"]] + list(col[1:]), coef), "coefficient_index": (row_ptr, col, [len(case["dict"])] + list(coef[1:])),
               "offsets_decrease": ([0, 5, 3] + list(row_ptr[3:]), col, coef), "offsets_overrun": (list(row_ptr[:-1]) + [len(col) + 1], col, coef)}
        for name, M in bad.items():
            rc, _outs, _sec = run(case, (M,) + tuple(case["mats"][1:]))
            res["refused"][name] = [rc, ctx.lib.vimz_last_error(ctx.h).decode()]
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"key origin kernels probe ok: {len(res['spmv'])} products, {res['seconds']:.1f} s")


def string_arrays(fixed_mul, string):
    return {name: fixed_mul(2 if name.endswith("g2") else 1, string[name]) for name in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")}


def rho_words(rho, rho_h):
    return np.frombuffer(b"".join(x.to_bytes(16, "little") for x in list(rho) + list(rho_h)), dtype="<u8").astype(np.uint64)


def origin_raw(ctx, circ, blob, arrays, rho, rho_h, n_tau_g1=None, n_pow=None):
    """the hook itself: {"rc", "result", "first_bad", "points" (hex), "message"}"""
    from vimz_amd import _lib, hip
    csr = Csr(circ["mats"])
    key = np.frombuffer(bytes(blob), dtype=np.uint8).copy()
    result, first, pts = C.c_uint32(0xFFFF), np.full(2, 7, dtype=np.uint64), np.full(112, 7, dtype=np.uint64)
    rc = ctx.lib.vimz_test_key_origin(ctx.h, csr.ptrs, csr.nnz, hip._ptr(to_words(circ["dict"])), len(circ["dict"]), circ["m"], circ["n_pub"], circ["n_c"], circ["logn"],
                                      hip._ptr(to_words([circ["pp_hash"]])), hip._ptr(key), key.size, hip._ptr(arrays["tau_g1"]), arrays["tau_g1"].shape[0] if n_tau_g1 is None else n_tau_g1,
                                      hip._ptr(arrays["tau_g2"]), hip._ptr(arrays["alpha_g1"]), hip._ptr(arrays["beta_g1"]), arrays["tau_g2"].shape[0] if n_pow is None else n_pow,
                                      hip._ptr(arrays["beta_g2"]), _lib.FORM_CANONICAL, hip._ptr(rho_words(rho, rho_h)), C.byref(result), hip._ptr(first), hip._ptr(pts))
    return {"rc": rc, "result": int(result.value), "first_bad": [int(first[0]), int(first[1])], "points": hex_of(pts), "message": ctx.lib.vimz_last_error(ctx.h).decode() if rc else ""}


def main_driver(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    ctx, fixed_mul = open_context()
    points = lambda group, scalars: [row.tobytes() for row in fixed_mul(group, scalars)]      # noqa: E731
    res = {"shapes": {}, "tampers": {}, "refused": {}}
    try:
        for shape in O.DRIVER_SHAPES:
            circ = O.circuit(*shape)
            string = O.string_of(circ["logn"])
            arrays = string_arrays(fixed_mul, string)
            rho, rho_h = O.fixed_rho(circ)
            key = O.derived_key(circ, string)
            blob = O.blob_of(key, points)
            t0 = time.time()
            got = origin_raw(ctx, circ, blob, arrays, rho, rho_h)
            got["seconds"] = time.time() - t0
            _bits, _first, want = O.verdict(key, circ, string, rho, rho_h)
            got["want_points"] = b"".join(points(g, [s])[0] for g, s in zip(O.POINT_GROUPS, want)).hex()
            after, _rec = hip.contribute_key(ctx, blob, delta=K.DELTAS[0], nonce=K.NONCES[0])
            got["contributed"] = origin_raw(ctx, circ, after.tobytes(), arrays, rho, rho_h)
            got["contributed_is_the_reference"] = after.tobytes() == O.blob_of(O.contributed(key, K.DELTAS[0]), points)
            res["shapes"]["/".join(str(x) for x in shape)] = got
        # the tampers, at one shape
        circ = O.circuit(*O.TAMPER_SHAPE)
        string = O.string_of(circ["logn"])
        arrays = string_arrays(fixed_mul, string)
        rho, rho_h = O.fixed_rho(circ)
        blob = O.blob_of(O.derived_key(circ, string), points)
        for name, t in O.tampers(circ, string).items():
            res["tampers"][name] = origin_raw(ctx, t["circuit"], O.apply_patch(blob, t, points), arrays, rho, rho_h)
        # a longer string serves the key; one a point short does not
        longer = string_arrays(fixed_mul, O.string_of(circ["logn"] + 1))
        res["longer_string"] = origin_raw(ctx, circ, blob, longer, rho, rho_h)
        n = circ["n"]
        off = arrays["alpha_g1"].copy(); off[1, 4] ^= np.uint64(1)
        res["refused"] = {"truncated": origin_raw(ctx, circ, blob[:-8], arrays, rho, rho_h), "wrong_magic": origin_raw(ctx, circ, K.put(blob, 0, b"VG16KEY1"), arrays, rho, rho_h),
                          "tau_g1_a_point_short": origin_raw(ctx, circ, blob, arrays, rho, rho_h, n_tau_g1=2 * n - 2), "powers_a_point_short": origin_raw(ctx, circ, blob, arrays, rho, rho_h, n_pow=n - 1),
                          "string_point_off_curve": origin_raw(ctx, circ, blob, dict(arrays, alpha_g1=off), rho, rho_h)}
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"key origin driver probe ok: {len(res['shapes'])} shapes, {len(res['tampers'])} tampers, {res['seconds']:.1f} s")


def decider_bench(ctx, fixed_mul):
    """the prover of the other decider probes, the string of its light decider's domain through a .ptau container, and the key a set-up from it saves"""
    from tests._decider_powers_gpu import ptau_bytes
    from tests._key_contrib_gpu import ALPHA, BETA, DELTA, TAU, DeciderBench
    from vimz_amd import hip, iden3
    bench = DeciderBench(ctx, fixed_mul)
    domain = C.c_uint64(0)
    ctx.lib.vimz_decider_domain.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    ctx._chk(ctx.lib.vimz_decider_domain(bench.cf.h, 1, C.byref(domain)))
    power = int(domain.value).bit_length() - 1
    sc = O.P.string_scalars(TAU, ALPHA, BETA, power)
    canon = {name: fixed_mul(2 if name.endswith("g2") else 1, sc[name]) for name in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")}
    ptau = ptau_bytes(power, canon)
    powers = iden3.read_ptau(ptau)
    dec = hip.Decider(bench.cf, powers=powers, light=True, delta=DELTA)
    return bench, powers, dec, ptau


def main_decider(out_path):
    t_start = time.time()
    from tests._key_contrib_gpu import ALPHA, BETA, DELTA, TAU
    from vimz_amd import _lib, hip, iden3
    ctx, fixed_mul = open_context()
    res = {}
    bench, powers, dec, ptau = decider_bench(ctx, fixed_mul)
    try:
        res["info"] = dec.info()
        key = dec.save_key()
        dec.close()
        sec = []
        res["saved_key"] = hip.verify_key_origin(bench.cf, powers, key, seconds=sec)
        res["seconds"] = list(sec)
        after, _rec = hip.contribute_key(ctx, key)
        res["contributed_key"] = hip.verify_key_origin(bench.cf, powers, after)
        # the trapdoor set-up's key with another alpha (its KZG point is the prover's SRS's, so tau stays)
        vp = C.c_void_p
        fn = ctx.lib.vimz_testing_decider_setup_trapdoor
        fn.argtypes = [vp, vp, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_double)]
        h, sec4 = vp(), (C.c_double * 4)()
        ctx._chk(fn(bench.cf.h, hip._ptr(bench.vk), 1, hip._ptr(to_words([TAU, ALPHA + 1, BETA, 1, DELTA])), C.byref(h), sec4))
        other = bench.trapdoor_decider(DELTA)    # the same trapdoor as the string: this key IS the derived one (and the wrapper's argtypes are set for the next)
        res["trapdoor_key_of_the_strings_scalars"] = hip.verify_key_origin(bench.cf, powers, other.save_key())
        other.close()
        wrapped = hip.Decider.__new__(hip.Decider)
        wrapped.prover, wrapped.ctx, wrapped.h, wrapped.light = bench.cf, ctx, h, True
        res["trapdoor_key_of_another_alpha"] = hip.verify_key_origin(bench.cf, powers, wrapped.save_key())
        wrapped.close()
        L = K.layout(key[:8 * K.KEY_IC].tobytes() + bytes(key.size - 8 * K.KEY_IC))
        info = res["info"]
        m, n_pub, n = info["wires"], info["public_inputs"], info["domain"]
        off = O.offsets(m, n_pub, n)
        assert off["l"] == L["off_lh"]
        poked = key.copy()
        i, j = off["l"] + 8 * 100000, off["l"] + 8 * 100001
        poked[8 * i:8 * i + 64] = key[8 * j:8 * j + 64]
        res["poked_l"] = hip.verify_key_origin(bench.cf, powers, poked)
        b2 = key[8 * off["b2"]:8 * (off["b2"] + 16 * m)].reshape(m, 128)
        live = np.flatnonzero(b2.any(axis=1))
        poked = key.copy()
        i, j = off["b2"] + 16 * int(live[5]), off["b2"] + 16 * int(live[6])
        poked[8 * i:8 * i + 128] = key[8 * j:8 * j + 128]
        res["poked_b2"] = hip.verify_key_origin(bench.cf, powers, poked)
        res["b2_identities"] = int(m - live.size)
        other_mode = key.copy()
        other_mode[48:56] = 0                    # the header says: a full decider's key
        res["other_mode"] = hip.verify_key_origin(bench.cf, powers, other_mode)
        # a bad string: refused by verify_powers before any key work; taken as given without it (the fault then shows as the string's, or in the equations)
        bad = dict(powers, tau_g1=np.array(powers["tau_g1"]))
        bad["tau_g1"][5] = powers["tau_g1"][6]
        try:
            hip.verify_key_origin(bench.cf, bad, key, verify_powers=True)
            res["bad_string_verified"] = [0, "accepted"]
        except _lib.VimzError as e:
            res["bad_string_verified"] = [e.code, str(e)]
        res["good_string_verified"] = hip.verify_key_origin(bench.cf, powers, key, verify_powers=True)
        try:
            hip.verify_key_origin(bench.cf, dict(powers, tau_g1=powers["tau_g1"][:2 * n - 2]), key)
            res["short_string"] = [0, "accepted"]
        except _lib.VimzError as e:
            res["short_string"] = [e.code, str(e)]
        res["problems"] = hip.keyorigin_problems(O.L | O.B2)
        # the command on those files
        # the command on files: it reads the string, builds its own prover for the step circuit and judges
        paths = {x: f"{out_path}.{x}" for x in ("ptau", "good.key", "bad.key")}
        with open(paths["ptau"], "wb") as fp:
            fp.write(ptau)
        key.tofile(paths["good.key"]); poked.tofile(paths["bad.key"])
        res["cli"] = {}
        for name, argv in (("good", ["verify-key", paths["ptau"], "hash", "HD", paths["good.key"]]), ("bad", ["verify-key", paths["ptau"], "hash", "HD", paths["bad.key"]]),
                           ("usage", ["verify-key", paths["ptau"]])):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
                rc = iden3._main(argv)
            res["cli"][name] = {"rc": rc, "stdout": buf.getvalue()}
        for p in paths.values():
            os.remove(p)
    finally:
        bench.close()
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["total_seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"key origin decider probe ok: domain {res['info']['domain']}, saved key {res['saved_key']}, stages {[round(x, 3) for x in res['seconds']]} s, {res['total_seconds']:.1f} s in all")


def main_measure(out_path):
    """what profiles/key_origin.txt records: vimz_decider_key_verify_origin's stage times beside vimz_decider_setup_from_powers' on the same string, alternating, four
    rounds (the first warms both up and is kept apart); the row histogram and the product's time on stderr (VIMZ_KEY_ORIGIN_STATS, the last round)"""
    t_start = time.time()
    from tests._key_contrib_gpu import DELTA
    from vimz_amd import hip
    ctx, fixed_mul = open_context()
    bench, powers, dec, _ptau = decider_bench(ctx, fixed_mul)
    res = {"verify_origin": [], "setup_from_powers": []}
    try:
        res["info"] = dec.info()
        key = dec.save_key()
        dec.close()
        for rnd in range(4):
            if rnd == 3:
                os.environ["VIMZ_KEY_ORIGIN_STATS"] = "1"
            sec = []
            t0 = time.time()
            res["verdict"] = hip.verify_key_origin(bench.cf, powers, key, seconds=sec)
            res["verify_origin"].append({"wall": time.time() - t0, "parts": list(sec)})
            os.environ.pop("VIMZ_KEY_ORIGIN_STATS", None)
            t0 = time.time()
            d = hip.Decider(bench.cf, powers=powers, light=True, delta=DELTA)
            res["setup_from_powers"].append({"wall": time.time() - t0, "parts": d.setup_seconds})
            d.close()
        # the full decider's histogram: a key whose header names the other mode makes the call synthesise that circuit (and refuse the key by its header)
        other_mode = key.copy()
        other_mode[48:56] = 0
        os.environ["VIMZ_KEY_ORIGIN_STATS"] = "1"
        try:
            res["other_mode"] = hip.verify_key_origin(bench.cf, powers, other_mode)
        finally:
            del os.environ["VIMZ_KEY_ORIGIN_STATS"]
    finally:
        bench.close()
        ctx.close()
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(json.dumps(res))


if __name__ == "__main__":
    {"kernels": main_kernels, "driver": main_driver, "decider": main_decider, "measure": main_measure}[sys.argv[1]](sys.argv[2])
