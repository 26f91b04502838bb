"""GPU half of tests/test_gpu_g16_powers_kernels.py, a process of its own with VIMZ_HIP_LIBRARY=testing (`python -m tests._g16_powers_gpu OUT.json`): the
same-scalar multiplication of a set-up from a powers-of-tau string (vimz_amd/csrc/g16_powers.hip) through vimz_test_g16_scale_points, over the cases of
tests/_g16_powers_ref.py.  Inputs are [s_i]G1 made by vimz_test_g16_fixed_mul, the expected outputs [k·s_i]G1 made the same way; vectors leave as the hex of
their little-endian words and nothing is judged here.  With a second argument `kzg` (tests/test_gpu_kzg_from_powers.py): hip.kzg_from_powers over a string of
known tau, made by the same hook and passed through a `.ptau` container and iden3.read_ptau.  Test infrastructure."""
import ctypes as C
import json
import sys
import time

import numpy as np

from tests import _g16_powers_ref as W
from tests._g16_kernels_gpu import hex_ints, hex_of, to_words
from tests._pairing import Q, R


def main(out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    lib = ctx.lib
    vp = C.c_void_p
    lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    lib.vimz_test_g16_scale_points.argtypes = [vp, vp, C.c_size_t, vp, vp]
    ptr = hip._ptr

    def fixed_mul(scalars):
        sc = to_words(scalars)
        out = np.full((len(scalars), 8), 7, dtype=np.uint64)
        ctx._chk(lib.vimz_test_g16_fixed_mul(ctx.h, 1, ptr(sc), len(scalars), ptr(out)))
        return out

    def scale_raw(points, k, n=None):
        out = np.full((len(points), 8), 7, dtype=np.uint64)
        return lib.vimz_test_g16_scale_points(ctx.h, ptr(points), len(points) if n is None else n, ptr(to_words([k])), ptr(out)), out

    res = {"scale": {}, "refused": {}}
    try:
        for n in W.SCALE_N:
            s = W.scale_points(n)
            pts = fixed_mul(s)
            for name, k in {**W.scale_scalars(), "zero": 0}.items():
                rc, out = scale_raw(pts, k)
                ctx._chk(rc)
                res["scale"][f"{n}/{name}"] = {"in": hex_of(pts), "out": hex_of(out), "want": hex_of(fixed_mul([k * x % R for x in s]))}
        pts = fixed_mul([1, 2])
        off, big = pts.copy(), pts.copy()
        off[1, 4] += np.uint64(1)                 # y + 1: not on the curve
        big[0, :4] = to_words([Q])[0]             # x = q: not below the modulus
        res["refused"] = {"n_0": scale_raw(pts, 3, n=0)[0], "scalar_r": scale_raw(pts, R)[0], "off_curve": scale_raw(off, 3)[0], "x_not_reduced": scale_raw(big, 3)[0]}
        res["accepted"] = scale_raw(pts, 3)[0]
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"g16 powers probe ok: {len(res['scale'])} scalings, {res['seconds']:.1f} s")


KZG_TAU, KZG_POWER = 0x1234567890ABCDEF1234567, 3
KZG_N = (2, 5, (2 << KZG_POWER) - 1)      # the least, an odd one, the whole string
KZG_SCALARS = [3, R - 1, 0, 1, 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF % R]


def main_kzg(out_path):
    from tests.test_ptau_host import write_ptau
    from vimz_amd import _lib, hip, iden3
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    lib = ctx.lib
    vp = C.c_void_p
    lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]

    def fixed_mul(group, scalars):
        out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
        ctx._chk(lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(to_words(scalars)), len(scalars), hip._ptr(out)))
        return out

    def refusal(fn):
        try:
            fn()
        except _lib.VimzError as e:
            return e.code
        return 0

    res = {"srs": {}, "commit": {}}
    try:
        n2 = 1 << KZG_POWER
        pw = [pow(KZG_TAU, k, R) for k in range(2 * n2 - 1)]
        g1 = [tuple(hex_ints(hex_of(row))) for row in fixed_mul(1, pw)]
        g2 = [(tuple(w[:2]), tuple(w[2:])) for w in (hex_ints(hex_of(row)) for row in fixed_mul(2, pw[:n2]))]
        res["tau_g1"], res["tau_g2_1"] = hex_of(fixed_mul(1, pw)), hex_of(fixed_mul(2, pw[1:2]))
        # (alpha, beta: any points of the right count — kzg_from_powers reads neither)
        powers = iden3.read_ptau(write_ptau(KZG_POWER, {"tau_g1": g1, "tau_g2": g2, "alpha_g1": g1[:n2], "beta_g1": g1[:n2], "beta_g2": g2[:1]}))
        for n in KZG_N:
            srs, vk = hip.kzg_from_powers(ctx, powers, n)
            res["srs"][str(n)] = {"n": srs.n, "points": hex_of(srs.download()), "vk": hex_of(vk), "vk_shape": list(vk.shape)}
            sc = (KZG_SCALARS * n)[:n]
            res["commit"][str(n)] = {"got": hex_of(ctx.msm(srs, to_words(sc))), "want": hex_of(fixed_mul(1, [sum(s * t for s, t in zip(sc, pw)) % R]))}
            srs.free()
        shifted = dict(powers, tau_g1=powers["tau_g1"][1:])
        big = np.array(powers["tau_g2"])
        big[1, :4] = to_words([Q])[0]
        res["refused"] = {"n_1": refusal(lambda: hip.kzg_from_powers(ctx, powers, 1)), "n_above": refusal(lambda: hip.kzg_from_powers(ctx, powers, 2 * n2)),
                          "not_generator": refusal(lambda: hip.kzg_from_powers(ctx, shifted, 2)),
                          "vk_not_reduced": refusal(lambda: hip.kzg_from_powers(ctx, dict(powers, tau_g2=big), 2)),
                          "one_g2_power": refusal(lambda: hip.kzg_from_powers(ctx, dict(powers, tau_g2=powers["tau_g2"][:1]), 2))}
    finally:
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"kzg_from_powers probe ok: {len(res['srs'])} keys")


if __name__ == "__main__":
    (main_kzg if sys.argv[2:] == ["kzg"] else main)(sys.argv[1])
