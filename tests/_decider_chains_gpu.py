"""GPU half of tests/test_gpu_decider_chains.py, a process of its own with VIMZ_HIP_LIBRARY=testing (`python -m tests._decider_chains_gpu OUT_DIR`).
Part 1: the cases of tests/_cf_chains_ref.py through vimz_test_decider_chains with where = 1 — k_cf_open_chains behind the launcher the prover calls; the
words leave as arrays (OUT_DIR/chains.npz), nothing is judged here.  Part 2: the full decider end to end with check 5's chains on the device
(VIMZ_DECIDER_CHAINS, vimz_testing_decider_witness) over the set-up of tests/_tamper_decider.py; what happened leaves as OUT_DIR/e2e.json.  Test infrastructure."""
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

from tests import _cf_chains_ref as R


def chains_part(ctx, out_dir):
    arrays, meta = {}, {}
    rc, _, _, H, _ = R.run_hook(ctx.lib, ctx.h, 1, R.multiples(1), [0])
    ctx._chk(rc)
    meta["H"] = [str(c) for c in H]
    runs = [(name, R.multiples(n), sc) for name, (n, sc) in R.cases().items()] + [(name, *R.degenerate_case(name, H)) for name in R.DEGENERATE]
    # (the degenerate launches once more over an honest G_0: the flag is the launch's own, not left over)
    runs.append(("G0_is_G", list(R.multiples(65)), R.degenerate_case(R.DEGENERATE[0], H)[1]))
    for name, gens, sc in runs:
        rc, w, e, h, bad = R.run_hook(ctx.lib, ctx.h, 1, gens, sc)
        ctx._chk(rc)
        meta[name] = {"bad": bad, "H": [str(c) for c in h]}
        if name in R.cases():
            arrays[name + "/wires"] = R._words(w); arrays[name + "/ends"] = R._words(e)
    np.savez(os.path.join(out_dir, "chains.npz"), **arrays)
    return meta


def e2e_part(ctx):
    from tests._oracle import from_limbs
    from tests.test_circuits import step_inputs
    from vimz_amd import _lib, hip
    from vimz_amd.circuit import Circuit
    res = {}
    srs, kzg_vk = hip.kzg_setup(ctx, 36000, seed=b"decider-chains srs")
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
    c = Circuit.for_resolution("hash", "HD")
    z0, inputs = step_inputs("hash")
    cf = hip.CycleFoldIVC(ctx, c, srs, ck2, max_batch=2)
    dec = light = None
    vp = C.c_void_p
    fn = ctx.lib.vimz_testing_decider_witness
    fn.argtypes = [vp, vp, C.c_int, vp, C.c_size_t]
    fn.restype = C.c_int64

    def witness(d, on_gpu):
        buf = np.zeros((d.info()["wires"], 4), dtype=np.uint64)
        got = fn(d.h, cf.h, int(on_gpu), hip._ptr(buf), buf.nbytes)
        if got < 0:
            ctx._chk(int(got))
        assert got == buf.nbytes, (got, buf.nbytes)
        return buf

    def prove(d, mode):
        os.environ["VIMZ_DECIDER_CHAINS"] = mode      # (read per call)
        try:
            return d.prove()
        finally:
            del os.environ["VIMZ_DECIDER_CHAINS"]

    try:
        cf.reset(z0); cf.fold(np.stack(inputs[:3]))
        assert cf.verify(3, z0) == 0
        dec = hip.Decider(cf, kzg_vk=kzg_vk, seed=b"decider-chains key")
        zh, zg = witness(dec, 0), witness(dec, 1)
        differ = np.flatnonzero((zh != zg).any(axis=1))
        res["witness_wires"] = int(zh.shape[0]); res["witness_first_difference"] = int(differ[0]) if differ.size else None
        res["witness_nonzero"] = int((zh != 0).any(axis=1).sum())
        lz = c.len_z
        words_g, pub_g, sec_g = prove(dec, "gpu")
        steps, a0, ai = pub_g[1], pub_g[2:2 + lz], pub_g[2 + lz:2 + 2 * lz]
        res["gpu_verify"] = dec.verify(steps, a0, ai, words_g)
        words_h, pub_h, sec_h = prove(dec, "host")
        res["host_verify"] = dec.verify(steps, a0, ai, words_h)
        res["public_inputs_equal"] = pub_g == pub_h
        res["seconds_gpu"] = sec_g; res["seconds_host"] = sec_h
        try:
            prove(dec, "neither")
            res["bad_switch"] = 0
        except _lib.VimzError as e:
            res["bad_switch"] = e.code
        # a CycleFold witness that no longer opens its commitment (nor satisfies its relation): no proof on the device path either
        vec = from_limbs(cf.export(1, hip.IX_RUNNING_Z))
        cf.poke(2, 5, (vec[5] + 1) % _lib.MODULUS[1])
        try:
            prove(dec, "gpu")
            res["poked"] = 0
        except _lib.VimzError as e:
            res["poked"] = e.code
        cf.poke(2, 5, vec[5])
        words_r, pub_r, _ = prove(dec, "gpu")
        res["restored_verify"] = dec.verify(steps, a0, ai, words_r); res["restored_public_inputs_equal"] = pub_r == pub_g
        # two proves and one assignment at once on the one decider, all with the device's chains: they take their turns (a wrong lock order would stop here for good)
        got = {}

        def job(name, f):
            try:
                got[name] = f()
            except BaseException as e:      # (reported by the parent test)
                got[name] = repr(e)

        os.environ["VIMZ_DECIDER_CHAINS"] = "gpu"
        jobs = [threading.Thread(target=job, args=(n, f), daemon=True) for n, f in (("prove_a", dec.prove), ("prove_b", dec.prove), ("witness", lambda: witness(dec, 1)))]
        for t in jobs:
            t.start()
        for t in jobs:
            t.join(timeout=300)
        del os.environ["VIMZ_DECIDER_CHAINS"]
        if any(t.is_alive() for t in jobs):
            sys.stderr.write("concurrent proves on one decider did not finish: " + ", ".join(sorted(got)) + " did\n"); sys.stderr.flush()
            os._exit(3)      # (the threads hold the library's locks: nothing can be closed)
        conc = {}
        for n in ("prove_a", "prove_b"):
            conc[n] = {"verify": dec.verify(steps, a0, ai, got[n][0]), "public_inputs_equal": got[n][1] == pub_g} if isinstance(got[n], tuple) else got[n]
        conc["witness_equal"] = bool(np.array_equal(got["witness"], zh)) if isinstance(got["witness"], np.ndarray) else got["witness"]
        res["concurrent"] = conc
        light = hip.Decider(cf, kzg_vk=kzg_vk, seed=b"decider-chains key", light=True)
        words_l, pub_l, sec_l = prove(light, "gpu")
        res["light_verify"] = light.verify(steps, a0, ai, words_l); res["seconds_light"] = sec_l
        res["err_unsat"] = _lib.ERR_UNSAT; res["err_invalid"] = _lib.ERR_INVALID
    finally:
        for o in (dec, light):
            if o is not None:
                o.close()
        cf.close(); srs.free(); ck2.free()
    return res


def main(out_dir):
    t0 = time.time()
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    try:
        meta = chains_part(ctx, out_dir)
        t1 = time.time()
        e2e = e2e_part(ctx)
    finally:
        ctx.close()
    with open(os.path.join(out_dir, "e2e.json"), "w") as fp:
        json.dump({"chains": meta, "e2e": e2e, "seconds": {"chains": t1 - t0, "e2e": time.time() - t1}}, fp)
    print(f"decider chains probe ok: {len(meta) - 1} launches in {t1 - t0:.1f} s, end to end {time.time() - t1:.1f} s; chains_gpu {e2e['seconds_gpu']['chains_gpu'] * 1e3:.1f} ms, "
          f"witness_host gpu {e2e['seconds_gpu']['witness_host']:.3f} s / host {e2e['seconds_host']['witness_host']:.3f} s")


if __name__ == "__main__":
    main(sys.argv[1])
