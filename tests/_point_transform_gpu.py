"""GPU half of tests/test_gpu_point_transform.py, a process of its own per group with VIMZ_HIP_LIBRARY=testing (`python -m tests._point_transform_gpu
{g1|g2|api} OUT.json`): the transform over points of a set-up from a powers-of-tau string (vimz_amd/csrc/g16_powers.hip).

g1, g2: g16_point_transform through vimz_test_g16_point_transform over the cases of tests/_g16_powers_ref.py.  Inputs are [s_k]G made by vimz_test_g16_fixed_mul,
the expected outputs [x_j]G made the same way.  api: vimz_powers_lagrange and hip.lagrange_from_powers over a string of known tau, alpha, beta made by the same
hook and passed through a `.ptau` container and iden3.read_ptau; the command-line form over the same file.  Vectors leave as the hex of their little-endian
words and nothing is judged here.  Test infrastructure."""
import ctypes as C
import json
import sys
import time

import numpy as np

from tests import _g16_powers_ref as W
from tests import _g16_ref as G
from tests._g16_kernels_gpu import hex_ints, hex_of, to_words
from tests._pairing import Q, R

API_TAU, API_ALPHA, API_BETA, API_POWER = 0x1234567890ABCDEF1234567, 0xFEDCBA987654321, 0x55AA55AA55AA77, 3
API_LOGN = (1, 3)
API_ARRAYS = (("tau_g1", 1), ("alpha_g1", 1), ("beta_g1", 1), ("tau_g2", 2))      # what lagrange_from_powers returns: name, group
API_EVALS = [5, R - 2, 0, 1, 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF % R, 7, 1 << 200, R - (1 << 130)]      # the first n of them


def open_context():
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    vp = C.c_void_p
    ctx.lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    ctx.lib.vimz_test_g16_point_transform.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    ctx.lib.vimz_powers_lagrange.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, vp, C.POINTER(C.c_double)]

    def fixed_mul(group, scalars):
        out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
        ctx._chk(ctx.lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(to_words(scalars)), len(scalars), hip._ptr(out)))
        return out
    return ctx, fixed_mul


def main_group(group, out_path):
    t_start = time.time()
    from vimz_amd import hip
    ctx, fixed_mul = open_context()

    def transform(points, logn, inverse, scaled):
        out = np.full(points.shape, 7, dtype=np.uint64)
        ctx._chk(ctx.lib.vimz_test_g16_point_transform(ctx.h, group, logn, inverse, scaled, hip._ptr(points), hip._ptr(out)))
        return out

    res = {"runs": {}}
    try:
        for logn in W.TRANSFORM_LOGN[group]:
            for name, s in W.transform_cases(logn).items():
                want = W.transform_expected(s, logn, name)
                pts = fixed_mul(group, s)
                got = {"fwd": transform(pts, logn, 0, 0)}
                if name in W.FULL_CASES:
                    got["inv"], got["inv_scaled"] = transform(pts, logn, 1, 0), transform(pts, logn, 1, 1)
                    got["back_unscaled"], got["back"] = transform(got["fwd"], logn, 1, 0), transform(got["fwd"], logn, 1, 1)
                assert set(got) == set(want)
                res["runs"][f"{logn}/{name}"] = {"in": hex_of(pts), "out": {k: hex_of(v) for k, v in got.items()}, "want": {k: hex_of(fixed_mul(group, want[k])) for k in got}}
    finally:
        ctx.close()
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"point transform probe (G{group}) ok: {len(res['runs'])} cases, {res['seconds']:.1f} s")


def main_api(out_path):
    t_start = time.time()
    from tests.test_ptau_host import write_ptau
    from vimz_amd import _lib, hip, iden3
    ctx, fixed_mul = open_context()
    lib = ctx.lib

    def lagrange_raw(group, points, n_points, form, logn, null=None):
        out = np.full((1 << API_POWER) * 16, 7, dtype=np.uint64)                  # room for the largest good call
        return lib.vimz_powers_lagrange(ctx.h, group, None if null == "points" else hip._ptr(points), n_points, form, logn,
                                        None if null == "out" else hip._ptr(out), None), out[:8 * min(group, 2) << API_POWER]

    res = {"bases": {}, "commit": {}}
    try:
        n2 = 1 << API_POWER
        sc = W.string_scalars(API_TAU, API_ALPHA, API_BETA, API_POWER)
        canon = {name: fixed_mul(group, sc[name]) for name, group in (("tau_g1", 1), ("alpha_g1", 1), ("beta_g1", 1), ("tau_g2", 2), ("beta_g2", 2))}
        g1_pts = lambda a: [tuple(hex_ints(hex_of(row))) for row in a]                                   # noqa: E731
        g2_pts = lambda a: [(tuple(w[:2]), tuple(w[2:])) for w in (hex_ints(hex_of(row)) for row in a)]      # noqa: E731
        res["string"] = {name: hex_of(a) for name, a in canon.items()}
        ptau = write_ptau(API_POWER, {name: (g2_pts if name.endswith("g2") else g1_pts)(a) for name, a in canon.items()})
        powers = iden3.read_ptau(ptau)
        for logn in API_LOGN:
            n = 1 << logn
            t0 = time.time()
            bases = hip.lagrange_from_powers(ctx, powers, logn)
            entry = {"seconds": time.time() - t0, "mont": {}, "canonical": {}, "want": {}, "want_closed": {}, "shape": {}}
            closed = W.lagrange_closed_form(API_TAU, logn)
            for (name, group), factor in zip(API_ARRAYS, (1, API_ALPHA, API_BETA, 1)):
                entry["mont"][name], entry["shape"][name] = hex_of(bases[name]), list(bases[name].shape)
                entry["canonical"][name] = hex_of(hip.powers_lagrange(ctx, group, canon[name], logn))      # the same inputs in canonical form, the ABI directly
                entry["want"][name] = hex_of(fixed_mul(group, W.lagrange(sc[name], logn)))
                entry["want_closed"][name] = hex_of(fixed_mul(group, [factor * x % R for x in closed]))
            res["bases"][str(logn)] = entry
            # a use that knows no scalars: a commitment to the polynomial with the evaluations e, by the Lagrange basis and by the coefficients
            e = API_EVALS[:n]
            lag = ctx.bases_upload(_lib.CURVE_BN254_G1, bases["tau_g1"], form=_lib.FORM_MONTGOMERY)
            srs, _vk = hip.kzg_from_powers(ctx, powers, n)
            res["commit"][str(logn)] = {"by_evaluations": hex_of(ctx.msm(lag, to_words(e))), "by_coefficients": hex_of(ctx.msm(srs, to_words(G.interpolate(e, logn))))}
            lag.free(); srs.free()
        # the command-line form, in this process: FILE.ptau LOGN OUT.npz (it opens a context of its own)
        ptau_path, npz_path = out_path + ".ptau", out_path + ".npz"
        with open(ptau_path, "wb") as fp:
            fp.write(ptau)
        rc = iden3._main(["lagrange", ptau_path, str(API_POWER), npz_path])
        with np.load(npz_path) as z:
            res["cli"] = {"rc": rc, "logn": int(z["logn"]), "arrays": {name: hex_of(z[name]) for name, _ in API_ARRAYS}, "usage_rc": iden3._main(["lagrange", ptau_path])}
        # the refusals of the ABI, then a good call
        g1, g2 = canon["tau_g1"][:n2].copy(), canon["tau_g2"].copy()
        off1, off2, big1, big2 = g1.copy(), g2.copy(), g1.copy(), g2.copy()
        off1[1, 4] += np.uint64(1); off2[1, 8] += np.uint64(1)                      # y + 1, y.c0 + 1: not on the curve
        big1[0, :4] = to_words([Q])[0]; big2[2, 4:8] = to_words([Q])[0]             # x = q, x.c1 = q: not below the modulus
        cn = _lib.FORM_CANONICAL
        res["refused"] = {
            "null_ctx": lib.vimz_powers_lagrange(None, 1, hip._ptr(g1), n2, cn, 3, hip._ptr(g1.copy()), None),
            "null_points": lagrange_raw(1, g1, n2, cn, 3, null="points")[0], "null_out": lagrange_raw(1, g1, n2, cn, 3, null="out")[0],
            "group_0": lagrange_raw(0, g1, n2, cn, 3)[0], "group_3": lagrange_raw(3, g2, n2, cn, 3)[0],
            "logn_0": lagrange_raw(1, g1, n2, cn, 0)[0], "logn_27": lagrange_raw(1, g1, n2, cn, 27)[0],
            "short_g1": lagrange_raw(1, g1, n2 - 1, cn, 3)[0], "short_g2": lagrange_raw(2, g2, n2 - 1, cn, 3)[0],
            "g1_not_reduced": lagrange_raw(1, big1, n2, cn, 3)[0], "g2_not_reduced": lagrange_raw(2, big2, n2, cn, 3)[0],
            "g1_off_curve": lagrange_raw(1, off1, n2, cn, 3)[0], "g2_off_curve": lagrange_raw(2, off2, n2, cn, 3)[0],
            "mont_not_reduced": lagrange_raw(1, big1, n2, _lib.FORM_MONTGOMERY, 3)[0]}
        rc1, out1 = lagrange_raw(1, g1, n2, cn, 3)
        rc2, out2 = lagrange_raw(2, g2, n2, cn, 3)
        res["accepted"] = {"g1": rc1, "g2": rc2, "g1_out": hex_of(out1), "g2_out": hex_of(out2)}
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"powers_lagrange probe ok: logn {list(res['bases'])}, {res['seconds']:.1f} s")


if __name__ == "__main__":
    what, out = sys.argv[1], sys.argv[2]
    if what == "api":
        main_api(out)
    else:
        main_group({"g1": 1, "g2": 2}[what], out)
