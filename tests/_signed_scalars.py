"""Vectors and the GPU half of tests/test_gpu_signed_scalars.py.  The MSM's switches are read once per process, so the test runs this
module twice (`python -m tests._signed_scalars OUT.json`, VIMZ_TUNE=signed_scalars=1 / 0) and compares what the two processes computed
with each other and with the CPU oracle, which it calls itself on the same vectors (built here, from fixed seeds)."""
import json
import random
import sys

MODULI = {
    0: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
    1: 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47,
    2: 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
    3: 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
}
SCALAR_FIELD = {0: 0, 1: 1, 2: 3, 3: 2}      # curve -> field of its scalars (tests/_oracle.py: CURVE_SCALAR)
N_LARGE = 40000                              # above MSM_SMALL_MAX (30 720): the sort / accumulate / combine / reduce pipeline
N_SMALL = 30720                              # the largest fused launch: 20 chunks a window
N_FIXED = 2000                               # small enough for tables of every multiple (189 KB a point)
VECTORS = ("mixed", "neg_small", "one_x", "bufm")


def boundary_values(p):
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    for k in range(p.bit_length()):
        if (1 << k) < p:
            vals += [1 << k, p - (1 << k)]
    return vals


def digits(s, c, p):
    """the signed digits of s (a Python-integer model of msm.hpp's for_each_digit: window c, K = ceil((bits of p + 1) / c) windows)"""
    half, carry, out = 1 << (c - 1), 0, []
    for w in range((p.bit_length() + c) // c):
        d = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        carry = 1 if d > half else 0
        out.append(d - (1 << c) if carry else d)
    return out


def entries(scalars, c, p, signed):
    """sort entries of an MSM over these scalars: the non-zero digits, of p - s where the signed loader takes s as a negative"""
    return sum(sum(1 for d in digits(p - s if signed and s > (p - 1) // 2 else s, c, p) if d) for s in scalars)


def vector(cid, kind, n=N_LARGE):
    """n scalars of curve `cid` as Python integers; every shorter case takes a prefix"""
    p = MODULI[SCALAR_FIELD[cid]]
    rng = random.Random(f"{cid}/{kind}")
    if kind == "mixed":        # the boundary values, repeated, among dense random scalars and 139-bit values of both signs
        b = boundary_values(p)
        out = []
        while len(out) < n:
            k = rng.random()
            out.append(rng.choice(b) if k < 0.4 else rng.randrange(p) if k < 0.7 else rng.getrandbits(139) if k < 0.85 else p - rng.getrandbits(139) - 1)
        out[:len(b)] = b
        return out[:n]
    def small():
        # a 139-bit x; on the BN254 fields one whose field element p - x has a digit in EVERY window of the c = 15 recoding (a random x has a zero
        # digit somewhere in about one case in 3 000, and the test counts entries exactly: 17 a scalar without the signed loader)
        while True:
            x = rng.getrandbits(139) | (1 << 138)
            if cid in (2, 3) or all(digits(p - x, 15, p)):
                return x
    if kind == "neg_small":    # every scalar p - (small)
        return [p - small() for _ in range(n)]
    if kind == "one_x":        # ONE value p - x everywhere: without the signed loader the heaviest buckets there can be
        return [p - small()] * n
    if kind == "bufm":         # the step rows' vector in its boolean-row form: 2(a - u) where the fresh bit is one, 0 elsewhere, a few dense rows
        steps = 64
        r = [(1 << 128) | rng.getrandbits(128) for _ in range(steps)]
        u = 1 + sum(r)
        out = []
        for _ in range(n):
            k = rng.random()
            if k < 0.45:
                out.append(0)
            elif k < 0.93:
                out.append((2 * (sum(x for x in r if rng.random() < 0.5) - u)) % p)
            else:
                out.append(rng.randrange(p))
        return out
    raise ValueError(kind)


def main(out_path):
    import numpy as np
    from tests import _oracle
    from tests._oracle import from_limbs, to_limbs
    from vimz_amd import hip
    orc = _oracle.load()
    ctx = hip.Context(0)
    res = {}
    try:
        for cid in (0, 1, 2, 3):
            fid = SCALAR_FIELD[cid]
            bases = orc.seq_bases(cid, N_LARGE)
            B = ctx.bases_upload(cid, bases)                        # no tables
            B15 = ctx.bases_upload(cid, bases).precompute(15)       # one shared bucket set, c = 15 (the bench's large MSM)
            B7 = ctx.bases_upload(cid, bases[:N_FIXED]).precompute(7)   # every multiple resident: k_msm_fixed
            try:
                for kind in VECTORS:
                    sc = vector(cid, kind)
                    limbs = to_limbs(sc)
                    v = ctx.vec_from_host(fid, limbs)
                    pt = lambda a: [int(x) for x in from_limbs(a)]      # noqa: E731
                    r = {}
                    r["large"] = pt(ctx.msm_vec(B, v))
                    r["large_entries"] = ctx.msm_last_profile()["entries"]
                    r["large_canonical_input"] = pt(ctx.msm(B, limbs))
                    r["large_c15"] = pt(ctx.msm_vec(B, v, window_bits=15))
                    r["large_c15_entries"] = ctx.msm_last_profile()["entries"]
                    r["large_tables15"] = pt(ctx.msm_vec(B15, v))
                    r["large_tables15_entries"] = ctx.msm_last_profile()["entries"]
                    r["large_tables15_split_ones"] = pt(ctx.msm_vec(B15, v, split_ones=True))
                    r["small"] = pt(ctx.msm_vec(B, v, n=N_SMALL))
                    r["small_canonical_input"] = pt(ctx.msm(B, np.ascontiguousarray(limbs[:N_SMALL])))
                    r["fixed_plain"] = pt(ctx.msm_vec(B, v, n=N_FIXED))
                    r["fixed_tables"] = pt(ctx.msm_vec(B7, v, n=N_FIXED))
                    v.free()
                    res[f"{cid}/{kind}"] = r
            finally:
                B.free(); B15.free(); B7.free()
    finally:
        ctx.close()
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print("signed-scalars probe ok", len(res))


if __name__ == "__main__":
    main(sys.argv[1])
