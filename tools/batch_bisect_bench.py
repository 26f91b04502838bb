#!/usr/bin/env python3
"""Measures what the bisection of a refused batch chunk costs and saves, for both batch verifiers, and writes profiles/batch_bisect.txt.  A record, not a gate.
Needs an MI355X.

Per verifier it measures, from the entries' own `fallback` seconds:
  * the per-member cost of the fallback without bisection (VIMZ_BATCH_NO_BISECT: every member of the refused chunk to the single verifier, as it is scheduled);
  * one subset evaluation at chunk/2 members: one bad member at place 0 with leaf = chunk/2 asks exactly TWO subsets of chunk/2 (L refused, R held) and verifies
    chunk/2 members singly, so  evaluation = (fallback(leaf = chunk/2) − fallback(no bisection)/2) / 2;
  * kappa = evaluation / per-member cost, and the default leaf it gives: the smallest power of two >= 8·kappa, at least 1;
  * the cases: one bad member, one bad member in every chunk, one chunk bad throughout — bisected and not.
usage: batch_bisect_bench.py [--what decider,compressed] [--rounds 3] [--transformation contrast] [--resolution HD] [--rows 4] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leaf_for(kappa):
    leaf = 1
    while leaf < 8 * kappa:
        leaf *= 2
    return leaf


def med(xs):
    return statistics.median(xs), min(xs), max(xs)


def fmt(m):
    return f"{m[0]:.4f} ({m[1]:.4f} .. {m[2]:.4f})"


def decider(ctx, rounds, lines, record):
    from tests._pairing import Q
    from tests.test_circuits import step_inputs
    from vimz_amd import _lib, calldata, hip
    from vimz_amd.circuit import Circuit
    srs, kzg_vk = hip.kzg_setup(ctx, 36000)
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
    cf = hip.CycleFoldIVC(ctx, Circuit.for_resolution("hash", "HD"), srs, ck2, max_batch=2)
    z0, inputs = step_inputs("hash")
    cf.reset(z0); cf.fold(np.stack(inputs[:2]))
    dec = hip.Decider(cf, kzg_vk=kzg_vk, light=True)
    _, d = calldata.decider_calldata(dec)
    kw = dec.key_words()
    good = (d["steps"], d["z0"], d["z_i"], list(d["words"]))
    bw = list(d["words"]); bw[16] = Q - bw[16]
    bad = (d["steps"], d["z0"], d["z_i"], bw)
    chunk = 256

    def run(handle, n, bad_at, **kw_):
        items = [bad if i in bad_at else good for i in range(n)]
        out = []
        for r in range(rounds + 1):
            st, sec = {}, {}
            t0 = time.perf_counter()
            words = hip.verify_decider_batch(handle, kw, items, stats=st, seconds=sec, **kw_)
            dt = time.perf_counter() - t0
            assert [w != 0 for w in words] == [i in bad_at for i in range(n)]
            if r:          # (the first round warms up)
                out.append((dt, sec["fallback"], sec["total"], st))
        return {"wall": med([o[0] for o in out]), "fallback": med([o[1] for o in out]), "total": med([o[2] for o in out]), "stats": out[0][3]}

    rec = record["decider"] = {}
    lines += [f"DECIDER — vimz_decider_verify_batch_ex, light hash decider's key, one valid 2-step proof repeated, a bad member has A -> −A (bit 3); chunk {chunk};",
              f"median (min .. max) seconds over {rounds} rounds after a warm-up; `fallback` and `total` are the entry's own seconds, `wall` the Python call's.", ""]
    for path, handle in (("device", ctx), ("host (ctx = None)", None)):
        off = run(handle, chunk, {0}, bisect=False)
        half = run(handle, chunk, {0}, leaf=chunk // 2)
        per_member = off["fallback"][0] / chunk
        evaluation = (half["fallback"][0] - off["fallback"][0] / 2) / 2
        kappa = evaluation / per_member
        rec[path] = {"per_member_s": per_member, "evaluation_s": evaluation, "kappa": kappa, "leaf": leaf_for(kappa), "no_bisect": off, "leaf_half": half, "cases": {}}
        lines += [f"{path}: one chunk of {chunk}, member 0 bad",
                  f"  no bisection        fallback {fmt(off['fallback'])} s = {chunk} single verifications over the threads: {1e3 * per_member:.3f} ms a member as scheduled",
                  f"  leaf = {chunk // 2}          fallback {fmt(half['fallback'])} s = 2 subset equations of {chunk // 2} members + {chunk // 2} single verifications  {half['stats']}",
                  f"  one subset equation at {chunk // 2} members: {1e3 * evaluation:.2f} ms;  kappa = {kappa:.2f};  smallest power of two >= 8·kappa: {leaf_for(kappa)}"]
        n = 1024
        cases = (("1 024 proofs, one bad", n, {517}), ("1 024 proofs, one bad in every chunk", n, {c * chunk + (37 * c + 5) % chunk for c in range(n // chunk)}),
                 ("1 024 proofs, one chunk bad throughout", n, set(range(chunk, 2 * chunk))))
        for name, size, bad_at in cases:
            a, b = run(handle, size, bad_at), run(handle, size, bad_at, bisect=False)
            rec[path]["cases"][name] = {"bisect": a, "no_bisect": b}
            lines.append(f"  {name}: bisected total {fmt(a['total'])} s, fallback {fmt(a['fallback'])} s {a['stats']};  not bisected total {fmt(b['total'])} s, fallback {fmt(b['fallback'])} s")
        clean = run(handle, n, set())
        rec[path]["clean_1024"] = clean
        lines += [f"  1 024 clean proofs: total {fmt(clean['total'])} s", ""]
    cf.close()


def compressed(ctx, a, lines, record):
    import bench
    from vimz_amd import folding, hip
    rows, z0 = bench.build_inputs(a.transformation, a.resolution)
    rows = np.stack(rows[:a.rows])
    circuit, params = folding.prepare_folding(ctx, a.transformation, a.resolution, backend="sonobe")
    ck2 = params.secondary_key()
    prover = hip.CycleFoldIVC(ctx, circuit, params.ck, ck2, max_batch=min(a.rows, folding.default_batch(circuit)))
    vk = hip.CycleFoldIVC(ctx, circuit, params.ck, ck2, max_batch=1)
    rec = record["compressed"] = {"config": f"{a.transformation}_step_{a.resolution}", "rows": a.rows, "cases": {}}
    try:
        prover.reset(z0); prover.fold(rows)
        blob, _ = prover.compress()
        good = np.array(blob, dtype=np.uint8)
        bad = good.copy(); bad[len(bad) - 32] ^= 1          # the last argument (Grumpkin): the chunk is refused on one curve
        assert vk.verify_compressed(blob, a.rows, z0) == 0
        t0 = time.perf_counter()
        assert vk.verify_compressed(blob, a.rows, z0) == 0
        t_single = time.perf_counter() - t0
        chunk = 32

        def run(n, bad_at, **kw):
            blobs = [bad if i in bad_at else good for i in range(n)]
            st = {}
            t0 = time.perf_counter()
            words, sec = vk.verify_compressed_batch(blobs, [a.rows] * n, [z0] * n, stats=st, **kw)
            dt = time.perf_counter() - t0
            assert [w != 0 for w in words] == [i in bad_at for i in range(n)]
            return {"wall": dt, "fallback": sec["fallback_s"], "seconds": sec, "stats": st}

        run(chunk, set())          # (a warm-up of the batch path)
        off = run(chunk, {0}, bisect=False)
        half = run(chunk, {0}, leaf=chunk // 2)
        per_member = off["fallback"] / chunk
        evaluation = (half["fallback"] - off["fallback"] / 2) / 2
        kappa1, kappa2 = evaluation / per_member, 2 * evaluation / per_member
        rec.update({"single_s": t_single, "per_member_s": per_member, "side_equation_s": evaluation, "kappa_one_curve": kappa1, "kappa_two_curves": kappa2, "leaf": leaf_for(kappa2),
                    "no_bisect": off, "leaf_half": half})
        lines += [f"COMPRESSED — vimz_cf_verify_batch_compressed_ex, {rec['config']}, one compressed \"cyclefold\" proof of {a.rows} rows repeated, a bad member has a bit of its last",
                  f"argument flipped; chunk {chunk}; ONE run a figure, wall-clock of the Python call and the entry's own `fallback` seconds; one single verification {1e3 * t_single:.1f} ms", "",
                  f"one chunk of {chunk}, member 0 bad",
                  f"  no bisection        wall {off['wall']:.3f} s, fallback {off['fallback']:.3f} s = {chunk} single verifications: {1e3 * per_member:.1f} ms a member",
                  f"  leaf = {chunk // 2}           wall {half['wall']:.3f} s, fallback {half['fallback']:.3f} s = 2 side equations of {chunk // 2} members + {chunk // 2} single verifications  {half['stats']}",
                  f"  one side equation at {chunk // 2} members: {1e3 * evaluation:.1f} ms;  kappa = {kappa1:.3f} (one curve asked), {kappa2:.3f} (both);  smallest power of two >= 8·kappa: {leaf_for(kappa2)}"]
        cases = (("32 proofs, one tampered", 32, {31}), ("256 proofs, one tampered in every chunk", 256, {c * chunk + (5 * c + 3) % chunk for c in range(8)}),
                 ("32 proofs, the chunk tampered throughout", 32, set(range(32))))
        for name, n, bad_at in cases:
            r = run(n, bad_at)
            rec["cases"][name] = {"bisect": r}
            line = f"  {name}: bisected wall {r['wall']:.3f} s, fallback {r['fallback']:.3f} s {r['stats']}"
            if n == 32:
                o = run(n, bad_at, bisect=False)
                rec["cases"][name]["no_bisect"] = o
                line += f";  not bisected wall {o['wall']:.3f} s, fallback {o['fallback']:.3f} s"
            lines.append(line)
        clean = run(256, set())
        rec["clean_256"] = clean
        lines += [f"  256 clean proofs: wall {clean['wall']:.3f} s", ""]
    finally:
        prover.close(); vk.close(); params.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="decider,compressed")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--transformation", default="contrast")
    ap.add_argument("--resolution", default="HD")
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bisect.txt"))
    a = ap.parse_args()
    from vimz_amd import hip
    ctx = hip.Context(0)
    lines, record = [], {}
    try:
        if "decider" in a.what:
            decider(ctx, a.rounds, lines, record)
        if "compressed" in a.what:
            compressed(ctx, a, lines, record)
    finally:
        ctx.close()
    text = "\n".join(lines) + "\n" + json.dumps(record) + "\n"
    with open(a.out, "w") as fp:
        fp.write(text)
    print(text)


if __name__ == "__main__":
    main()
