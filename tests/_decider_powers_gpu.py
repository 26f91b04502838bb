"""GPU half of tests/test_gpu_decider_from_powers.py, a process of its own per part with VIMZ_HIP_LIBRARY=testing (`python -m tests._decider_powers_gpu
{g1|g2|setup} OUT.json`): the column sums, the h query and the decider's set-up from a powers-of-tau string (vimz_amd/csrc/g16_powers.hip, groth16.hip).

g1: g16_column_sums through vimz_test_g16_column_sums over every case of tests/_g16_powers_ref.colsum_cases() in G1, and g16_h_query through vimz_test_g16_h_query.
g2: the column sums in G2 over G2_CASES.  Inputs are [s_r]G made by vimz_test_g16_fixed_mul, the expected outputs [x_j]G made the same way.
setup: the light decider of the hash step set up twice — from a string of known (tau, alpha, beta) with a given delta (the string made by the same hook, passed
through a `.ptau` container and iden3.read_ptau), and by the trapdoor set-up with (tau, alpha, beta, 1, delta) — their saved keys, a proof under the first key, and
the refusals; the second call's seconds[] with VIMZ_DECIDER_POWERS_STATS set (the library's lines on this process's stderr); the command line
(`python -m vimz_amd.iden3 decider-key`, in this process) and `tools/e2e.py ... --ptau` (a process of its own) over the same container.  Vectors leave as the hex of their little-endian words and nothing is judged here.  Test infrastructure."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np

from tests import _g16_powers_ref as W
from tests._g16_kernels_gpu import from_words, hex_of, to_words
from tests._pairing import Q, R

G2_CASES = ("1/33", "65/mixed", "64/empty")
HQ_N = (2, 64, 128)
HQ_TAU, HQ_DELTA = 0x1234567890ABCDEF1234567, 0x7654321FEDCBA9876543
TAU, ALPHA, BETA, DELTA = 0x2545F4914F6CDD1D0123456789ABCDEF, 0xFEDCBA987654321, 0x55AA55AA55AA77, 0x1B873593CC9E2D51
N_SRS, STEPS = 36000, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hq_cases(n):
    """name -> (input scalars, delta): the powers of a known tau; delta = 1; an identity among the inputs — as the minuend P[j + n] of output 0 (`identity`), and as
    the subtrahend P[j] of output 0 (`identity_low`: pt_diff then has nothing to negate)"""
    s = [pow(HQ_TAU, k, R) for k in range(2 * n - 1)]
    hole, low = list(s), list(s)
    hole[n] = 0
    low[0] = 0
    return {"plain": (s, HQ_DELTA), "delta_one": (s, 1), "identity": (hole, HQ_DELTA), "identity_low": (low, HQ_DELTA)}


def hq_expected(s, delta, n):
    dinv = pow(delta, -1, R)
    return [(s[j + n] - s[j]) * dinv % R for j in range(n - 1)]


def open_context():
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    vp = C.c_void_p
    ctx.lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    ctx.lib.vimz_test_g16_column_sums.argtypes = [vp, C.c_int, vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, vp, C.c_int, vp]
    ctx.lib.vimz_test_g16_h_query.argtypes = [vp, vp, C.c_size_t, vp, vp]

    def fixed_mul(group, scalars):
        out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
        ctx._chk(ctx.lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(to_words(scalars)), len(scalars), hip._ptr(out)))
        return out
    return ctx, fixed_mul


def main_group(group, out_path):
    t_start = time.time()
    from vimz_amd import _lib, hip
    ctx, fixed_mul = open_context()
    res = {"colsum": {}, "hq": {}}
    try:
        cases = W.colsum_cases()
        for name in (cases if group == 1 else G2_CASES):
            case = W.colsum_case(*cases[name])
            row_ptr, col, coef = (np.array(x, dtype=np.uint32) for x in case["csr"])
            col, coef = (x if x.size else np.zeros(1, dtype=np.uint32) for x in (col, coef))
            pts, dic = fixed_mul(group, case["scalars"]), to_words(case["dict"])
            out = np.full((case["n_cols"], 8 * group), 7, dtype=np.uint64)
            t0 = time.time()
            ctx._chk(ctx.lib.vimz_test_g16_column_sums(ctx.h, group, hip._ptr(row_ptr), hip._ptr(col), hip._ptr(coef), case["n_rows"], case["n_cols"], hip._ptr(dic),
                                                       len(case["dict"]), hip._ptr(pts), _lib.FORM_CANONICAL, hip._ptr(out)))
            res["colsum"][name] = {"out": hex_of(out), "want": hex_of(fixed_mul(group, W.colsum_expected(case))), "seconds": time.time() - t0}
        if group == 1:
            for n in HQ_N:
                for name, (s, delta) in hq_cases(n).items():
                    out = np.full((n - 1, 8), 7, dtype=np.uint64)
                    ctx._chk(ctx.lib.vimz_test_g16_h_query(ctx.h, hip._ptr(fixed_mul(1, s)), n, hip._ptr(to_words([pow(delta, -1, R)])), hip._ptr(out)))
                    res["hq"][f"{n}/{name}"] = {"out": hex_of(out), "want": hex_of(fixed_mul(1, hq_expected(s, delta, n)))}
    finally:
        ctx.close()
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"column sums probe (G{group}) ok: {len(res['colsum'])} cases, {len(res['hq'])} h queries, {res['seconds']:.1f} s")


def ptau_bytes(power, canon):
    """snarkjs's container around canonical point arrays: every coordinate into the file's Montgomery form"""
    def section(a):
        raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
        return b"".join((int.from_bytes(raw[i:i + 32], "little") * (1 << 256) % Q).to_bytes(32, "little") for i in range(0, len(raw), 32))
    secs = {1: struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, power)}
    for t, name in {2: "tau_g1", 3: "tau_g2", 4: "alpha_g1", 5: "beta_g1", 6: "beta_g2"}.items():
        secs[t] = section(canon[name])
    out = b"ptau" + struct.pack("<II", 1, len(secs))
    for t in sorted(secs):
        out += struct.pack("<IQ", t, len(secs[t])) + secs[t]
    return out


def main_setup(out_path):
    t_start = time.time()
    from tests.test_circuits import step_inputs
    from vimz_amd import _lib, hip, iden3
    from vimz_amd.circuit import Circuit
    ctx, fixed_mul = open_context()
    vp = C.c_void_p
    res = {"refused": {}}
    c = Circuit.for_resolution("hash", "HD")
    z0, inputs = step_inputs("hash")
    z0_in = z0
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
    srs0 = ctx.bases_upload(_lib.CURVE_BN254_G1, fixed_mul(1, [pow(TAU, k, R) for k in range(N_SRS)]))
    cf = hip.CycleFoldIVC(ctx, c, srs0, ck2, max_batch=2)
    dec_td = dec_pw = srs = cf2 = None
    try:
        cf.reset(z0); cf.fold(np.stack(inputs[:STEPS]))
        # the trapdoor set-up with the string's scalars and gamma = 1
        fn = ctx.lib.vimz_testing_decider_setup_trapdoor
        fn.argtypes = [vp, vp, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_double)]
        vk, td, h, sec4 = fixed_mul(2, [TAU]).reshape(4, 4), to_words([TAU, ALPHA, BETA, 1, DELTA]), vp(), (C.c_double * 4)()
        t0 = time.time()
        ctx._chk(fn(cf.h, hip._ptr(vk), 1, hip._ptr(td), C.byref(h), sec4))
        dec_td = hip.Decider.__new__(hip.Decider)      # (as Decider.load_key wraps a handle)
        dec_td.prover, dec_td.ctx, dec_td.h, dec_td.light = cf, ctx, h, True
        ctx.lib.vimz_decider_free.argtypes, ctx.lib.vimz_decider_free.restype, ctx.lib.vimz_decider_info.argtypes = [vp], None, [vp, vp]
        ctx.lib.vimz_decider_verify.argtypes = [vp, C.c_uint64, vp, vp, vp, C.POINTER(C.c_uint32)]
        res["trapdoor_seconds"] = {"wall": time.time() - t0, "parts": list(sec4)}
        info = dec_td.info()
        n = info["domain"]
        power = n.bit_length() - 1
        # the string of that power: made on the GPU by the fixed-base hook, through a .ptau container
        sc = W.string_scalars(TAU, ALPHA, BETA, power)
        canon = {name: fixed_mul(2 if name.endswith("g2") else 1, sc[name]) for name in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")}
        ptau = ptau_bytes(power, canon)
        powers = iden3.read_ptau(ptau)
        srs, kzg_vk = hip.kzg_from_powers(ctx, powers, N_SRS)
        res["srs_is_the_strings"] = bool(np.array_equal(srs.download(), srs0.download())) and hex_of(kzg_vk) == hex_of(vk)
        t0 = time.time()
        dec_pw = hip.Decider(cf, powers=powers, light=True, delta=DELTA)
        res["powers_seconds"] = {"wall": time.time() - t0, "parts": dec_pw.setup_seconds}
        blob_pw, blob_td = dec_pw.save_key(), dec_td.save_key()
        res["info"], res["info_powers"] = info, dec_pw.info()
        res["key"] = {"bytes": [int(blob_pw.size), int(blob_td.size)], "sha256": [hashlib.sha256(blob_pw.tobytes()).hexdigest(), hashlib.sha256(blob_td.tobytes()).hexdigest()],
                      "identical": bool(np.array_equal(blob_pw, blob_td)),
                      "first_difference": None if np.array_equal(blob_pw, blob_td) or blob_pw.size != blob_td.size else int(np.flatnonzero(blob_pw != blob_td)[0])}
        # a proof under the first key
        words, pub, _ = dec_pw.prove()
        lz = c.len_z
        z0, zi = pub[2:2 + lz], pub[2 + lz:2 + 2 * lz]
        res["proof"] = {"words": [hex(w) for w in words], "public_inputs": [hex(x) for x in pub], "steps": STEPS, "z0": [hex(int(x)) for x in z0], "z_i": [hex(int(x)) for x in zi],
                        "verify": dec_pw.verify(STEPS, z0, zi, words), "verify_trapdoor_key": dec_td.verify(STEPS, z0, zi, words),
                        "verify_changed": dec_pw.verify(STEPS, z0, zi, words[:16] + [Q - words[16]] + words[17:]),
                        "key_words": hex_of(dec_pw.key_words())}
        # the second of two calls, and the production entry (delta from the OS): another key, under which a proof verifies
        os.environ["VIMZ_DECIDER_POWERS_STATS"] = "1"      # (read per call: the plans' shapes and the device memory, on stderr)
        try:
            dec2 = hip.Decider(cf, powers=powers, light=True)
        finally:
            del os.environ["VIMZ_DECIDER_POWERS_STATS"]
        try:
            res["second_call_seconds"] = dec2.setup_seconds
            w2, _, _ = dec2.prove()
            res["os_delta"] = {"verify": dec2.verify(STEPS, z0, zi, w2), "verify_under_fixed_delta_key": dec_pw.verify(STEPS, z0, zi, w2),
                               "same_key": bool(np.array_equal(dec2.save_key(), blob_pw))}
        finally:
            dec2.close()

        # the refusals, each with its message
        def refusal(fn):
            try:
                d = fn()
            except _lib.VimzError as e:
                return [e.code, str(e)]
            d.close()
            return [0, "accepted"]

        def changed(name, row, array):
            a = np.array(powers[name])
            a[row] = array
            return dict(powers, **{name: a})
        mont = lambda a: np.frombuffer(b"".join((x * (1 << 256) % Q).to_bytes(32, "little") for x in from_words(a)), dtype="<u8").astype(np.uint64)      # noqa: E731
        off = np.array(powers["alpha_g1"][3])
        off[4] ^= np.uint64(1)
        res["refused"] = {
            "short_string": refusal(lambda: hip.Decider(cf, powers=dict(powers, tau_g1=powers["tau_g1"][:2 * n - 2]), light=True)),
            "short_powers": refusal(lambda: hip.Decider(cf, powers=dict(powers, beta_g1=powers["beta_g1"][:n - 1]), light=True)),
            "not_generator": refusal(lambda: hip.Decider(cf, powers=changed("tau_g1", 0, powers["tau_g1"][1]), light=True)),
            "tau_g2_of_another_tau": refusal(lambda: hip.Decider(cf, powers=changed("tau_g2", 1, mont(fixed_mul(2, [TAU + 1]))), light=True)),
            "beta_g2_of_another_beta": refusal(lambda: hip.Decider(cf, powers=changed("beta_g2", 0, mont(fixed_mul(2, [BETA + 1]))), light=True)),
            "alpha_is_zero": refusal(lambda: hip.Decider(cf, powers=changed("alpha_g1", 0, np.zeros(8, dtype=np.uint64)), light=True)),
            "off_curve": refusal(lambda: hip.Decider(cf, powers=changed("alpha_g1", 3, off), light=True)),
            "powers_and_kzg_vk": refusal(lambda: hip.Decider(cf, powers=powers, kzg_vk=kzg_vk, light=True)),
        }
        # a prover whose SRS is another tau's: the string is sound, the pair is not
        srs_other = ctx.bases_upload(_lib.CURVE_BN254_G1, fixed_mul(1, [pow(TAU + 1, k, R) for k in range(N_SRS)]))
        cf2 = hip.CycleFoldIVC(ctx, c, srs_other, ck2, max_batch=2)
        try:
            res["refused"]["srs_of_another_tau"] = refusal(lambda: hip.Decider(cf2, powers=powers, light=True))
        finally:
            cf2.close(); srs_other.free()
        # the command line over the same container: decider-key writes a key that loads into a prover made as it makes its own, and proves
        ptau_path, key_path = out_path + ".ptau", out_path + ".key"
        with open(ptau_path, "wb") as fp:
            fp.write(ptau)
        rc = iden3._main(["decider-key", ptau_path, "hash", "HD", key_path, "--light"])
        from vimz_amd import folding
        circuit_k, params_k = folding.prepare_folding(ctx, "hash", "HD", window_tables=0, backend="sonobe", powers=powers)
        cfk = hip.CycleFoldIVC(ctx, circuit_k, params_k.ck, params_k.secondary_key(), max_batch=1)
        dec_k = None
        try:
            cfk.reset(z0_in); cfk.fold(np.stack(inputs[:STEPS]))
            blob_k = np.fromfile(key_path, dtype=np.uint8)
            dec_k = hip.Decider.load_key(cfk, blob_k)
            wk, pk, _ = dec_k.prove()
            res["cli"] = {"rc": rc, "bytes": int(blob_k.size), "info": dec_k.info(), "verify": dec_k.verify(STEPS, pk[2:2 + lz], pk[2 + lz:2 + 2 * lz], wk),
                          "alpha_beta_gamma_are_the_strings": bool(np.array_equal(dec_k.key_words()[5:5 + 8 + 32], dec_pw.key_words()[5:5 + 8 + 32]))}
        finally:
            if dec_k is not None:
                dec_k.close()
            cfk.close(); params_k.free()
        # tools/e2e.py --ptau: the Sonobe path end to end over the string, with the light decider
        e2e = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "e2e.py"), "hash", "HD", "1", "cyclefold", "-", "--ptau", ptau_path], cwd=ROOT, capture_output=True, text=True,
                             timeout=300, env={**os.environ, "VIMZ_E2E_DECIDER": "light", "VIMZ_HIP_LIBRARY": ""})
        line = e2e.stdout.strip().splitlines()[-1] if e2e.stdout.strip() else ""
        res["e2e"] = {"rc": e2e.returncode, "stderr": e2e.stderr[-1500:], "json": json.loads(line) if line.startswith("{") else None}
    finally:
        for d in (dec_pw, dec_td):
            if d is not None:
                d.close()
        cf.close(); srs0.free(); ck2.free()
        if srs is not None:
            srs.free()
        ctx.close()
    res["invalid"] = _lib.ERR_INVALID
    res["seconds"] = time.time() - t_start
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"decider from powers probe ok: domain {res['info']['domain']}, keys identical: {res['key']['identical']}, set-up {res['powers_seconds']['wall']:.2f} s "
          f"(trapdoor {res['trapdoor_seconds']['wall']:.2f} s), {res['seconds']:.1f} s in all")


if __name__ == "__main__":
    what, out = sys.argv[1], sys.argv[2]
    if what == "setup":
        main_setup(out)
    else:
        main_group({"g1": 1, "g2": 2}[what], out)
