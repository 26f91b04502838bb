"""GPU half of tests/test_gpu_mlkzg_kernels.py and tests/test_gpu_mlkzg.py, a process of its own per part with VIMZ_HIP_LIBRARY=testing
(`python -m tests._mlkzg_gpu {kernels|open|cf} OUT.json`): the multilinear KZG opening (vimz_amd/csrc/mlkzg.hip).

kernels: every stage through its hook (vimz_test_mlkzg_*) on the cases below, whose sizes come from the hook's own constants — the evaluation and the division at
         each side of the chunk, block and cross-block boundaries for u = 0, 1, r − 1 and random ones, the fold and the batching at ℓ = 1, 2, 3 and the least ℓ past
         one block of chunks for x_k = 0, 1 and random ones.
open:    vimz_mlkzg_open end to end over an SRS of a tau chosen here (its powers by vimz_test_g16_fixed_mul), beside vimz_msm_vec's commitment and the verifier's
         verdicts on the proof, on eval + 1 and on flipped words; the refusals.
cf:      one CycleFold proof over the hash step with a seeded SRS, and a merged proof of one segment: vimz_cf_mlkzg_open / vimz_cf_merged_mlkzg_open beside the
         exported instance and running vectors.
Vectors leave as the hex of their little-endian words and nothing is judged here.  Test infrastructure."""
import ctypes as C
import json
import random
import sys

import numpy as np

from tests._g16_kernels_gpu import hex_of, to_words
from tests._pairing import Q, R

TAU = 0x0FEDCBA987654321123456789ABCDEF00112233445566778899AABBCCDDEEFF % R
OPEN_LOGN = (1, 2, 3, 10, 13)
U_RANDOM = (0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R, 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R)
EVAL_U = (0, 1, R - 1, U_RANDOM[0])
DIVIDE_U = ((0, 1, R - 1), (U_RANDOM[0], U_RANDOM[1], R - 2))
X_KINDS = ("zero", "one", "random")


def sizes(block, chunk):
    bc = block * chunk
    return [1, 2, chunk - 1, chunk, chunk + 1, bc - 1, bc, bc + 1, 2 * bc + 3]


def fold_logns(block, chunk):
    return [1, 2, 3, (block * chunk).bit_length()]


def coeffs(n, label="poly"):
    rng = random.Random(f"mlkzg/{label}/{n}")
    v = [rng.randrange(R) for _ in range(n)]
    v[-1] = R - 1
    if n > 2:
        v[1] = 0
    return v


def point(logn, kind="random", label="x"):
    rng = random.Random(f"mlkzg/{label}/{logn}")
    return [{"zero": 0, "one": 1}.get(kind, rng.randrange(R)) for _ in range(logn)]


def level_lengths(n0, nlevels):
    return [n0 >> k for k in range(nlevels)]


def open_sizes(logn):
    return sorted({1, (1 << logn) - 1, 1 << logn})


def cf_logn(n):
    """the least logn >= 1 with 2^logn >= n"""
    return max(1, (n - 1).bit_length())


def _hooks(ctx):
    lib, vp, sz, u32 = ctx.lib, C.c_void_p, C.c_size_t, C.c_uint32
    lib.vimz_test_mlkzg_shape.argtypes = [vp]
    lib.vimz_test_mlkzg_fold.argtypes = [vp, vp, u32, vp, vp]
    lib.vimz_test_mlkzg_eval3.argtypes = [vp, vp, sz, u32, vp, vp]
    lib.vimz_test_mlkzg_batch.argtypes = [vp, vp, sz, u32, vp, vp]
    lib.vimz_test_mlkzg_divide.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.vimz_test_g16_fixed_mul.argtypes = [vp, C.c_int, vp, sz, vp]
    return lib


def main_kernels(ctx, hip, res):
    lib, ptr = _hooks(ctx), hip._ptr
    shape = np.zeros(2, dtype=np.uint32)
    ctx._chk(lib.vimz_test_mlkzg_shape(ptr(shape)))
    block, chunk = int(shape[0]), int(shape[1])
    res["shape"] = [block, chunk]

    def eval3(levels, n0, nlevels, r):
        out = np.full((3 * nlevels, 4), 7, dtype=np.uint64)
        ctx._chk(lib.vimz_test_mlkzg_eval3(ctx.h, ptr(to_words(levels)), n0, nlevels, ptr(to_words([r])), ptr(out)))
        return hex_of(out)

    res["eval"], res["divide"], res["fold"], res["batch"] = {}, {}, {}, {}
    for n in sizes(block, chunk):
        p = to_words(coeffs(n))
        for u in EVAL_U:
            res["eval"][f"{n}/{u}"] = eval3(coeffs(n), n, 1, u)
        nch = -(-n // chunk)
        for k, us in enumerate(DIVIDE_U):
            quot, rem = np.full((3 * max(n - 1, 1), 4), 7, dtype=np.uint64), np.full((3, 4), 7, dtype=np.uint64)
            cout, cin = np.full((3 * nch, 4), 7, dtype=np.uint64), np.full((3 * nch, 4), 7, dtype=np.uint64)
            ctx._chk(lib.vimz_test_mlkzg_divide(ctx.h, ptr(p), n, ptr(to_words(us)), ptr(quot), ptr(rem), ptr(cout), ptr(cin)))
            res["divide"][f"{n}/{k}"] = {"quot": hex_of(quot[:3 * (n - 1)]), "rem": hex_of(rem), "carry": hex_of(cout), "carry_in": hex_of(cin)}
    n0 = sizes(block, chunk)[-1]
    lv = [c for k, ln in enumerate(level_lengths(n0, 3)) for c in coeffs(ln, f"levels{k}")]
    res["eval_levels"] = eval3(lv, n0, 3, U_RANDOM[1])
    for logn in fold_logns(block, chunk):
        N = 1 << logn
        for kind in X_KINDS:
            out = np.full((2 * N - 1, 4), 7, dtype=np.uint64)
            ctx._chk(lib.vimz_test_mlkzg_fold(ctx.h, ptr(to_words(coeffs(N, "fold"))), logn, ptr(to_words(point(logn, kind))), ptr(out)))
            res["fold"][f"{logn}/{kind}"] = hex_of(out)
        lv = [c for k in range(logn) for c in coeffs(N >> k, f"batch{k}")]
        for name, q in (("random", U_RANDOM[0]), ("minus_one", R - 1), ("zero", 0)):
            out = np.full((N, 4), 7, dtype=np.uint64)
            ctx._chk(lib.vimz_test_mlkzg_batch(ctx.h, ptr(to_words(lv)), N, logn, ptr(to_words([q])), ptr(out)))
            res["batch"][f"{logn}/{name}"] = hex_of(out)
    bad = np.zeros((4, 4), dtype=np.uint64)
    res["refused"] = {"eval_n_0": lib.vimz_test_mlkzg_eval3(ctx.h, ptr(bad), 0, 1, ptr(bad), ptr(bad)),
                      "eval_element_r": lib.vimz_test_mlkzg_eval3(ctx.h, ptr(to_words([R])), 1, 1, ptr(bad), ptr(bad)),
                      "divide_n_0": lib.vimz_test_mlkzg_divide(ctx.h, ptr(bad), 0, ptr(bad), ptr(bad), ptr(bad), None, None),
                      "fold_logn_0": lib.vimz_test_mlkzg_fold(ctx.h, ptr(bad), 0, ptr(bad), ptr(bad))}


def _fixed_mul(ctx, hip, group, scalars):
    out = np.full((len(scalars), 8 * group), 7, dtype=np.uint64)
    ctx._chk(ctx.lib.vimz_test_g16_fixed_mul(ctx.h, group, hip._ptr(to_words(scalars)), len(scalars), hip._ptr(out)))
    return out


def _refusal(fn):
    from vimz_amd import _lib
    try:
        fn()
    except _lib.VimzError as e:
        return e.code
    return 0


def main_open(ctx, hip, res):
    from vimz_amd import _lib
    lib = _hooks(ctx)
    top = max(OPEN_LOGN)
    pw = [pow(TAU, k, R) for k in range(1 << top)]
    srs = ctx.bases_upload(_lib.CURVE_BN254_G1, _fixed_mul(ctx, hip, 1, pw))
    vk = _fixed_mul(ctx, hip, 2, [TAU]).reshape(-1)
    res["vk"], res["open"] = hex_of(vk), {}

    def flip(words, at, modulus=R):
        """the element at word `at` with its lowest bit flipped — or less one where that would leave the range (an evaluation r − 1 of the vectors above)"""
        v = sum(int(words[at + k]) << (64 * k) for k in range(4))
        out = words.copy()
        out[at:at + 4] = to_words([v ^ 1 if v ^ 1 < modulus else v - 1])[0]
        return out

    for logn in OPEN_LOGN:
        x = point(logn)
        for n in open_sizes(logn):
            vec = ctx.vec_from_host(_lib.FIELD_BN254_FR, to_words(coeffs(n, "open")))
            sec = {}
            comm, ev, proof = ctx.mlkzg_open(srs, vec, x, seconds=sec)
            e, w = 8 * (logn - 1), 8 * (logn - 1) + 12 * logn
            res["open"][f"{logn}/{n}"] = {
                "comm": hex_of(comm), "msm_vec": hex_of(ctx.msm_vec(srs, vec)), "eval": ev, "proof": hex_of(proof), "seconds": sec,
                "verdicts": {"untouched": hip.mlkzg_verify(vk, comm, x, ev, proof), "eval + 1": hip.mlkzg_verify(vk, comm, x, (ev + 1) % R, proof),
                             "E_r flipped": hip.mlkzg_verify(vk, comm, x, ev, flip(proof, e)), "E_r2[0] flipped": hip.mlkzg_verify(vk, comm, x, ev, flip(proof, e + 8 * logn)),
                             "W flipped": hip.mlkzg_verify(vk, comm, x, ev, flip(proof, w + 8, Q))}}
            vec.free()
    # a slice of a longer vector
    vec = ctx.vec_from_host(_lib.FIELD_BN254_FR, to_words([5, 6, 7] + coeffs(7, "open") + [9]))
    comm, ev, proof = ctx.mlkzg_open(srs, vec, point(3), n=7, offset=3)
    res["slice"] = {"comm": hex_of(comm), "eval": ev, "proof": hex_of(proof)}
    # the refusals
    fq = ctx.vec_from_host(_lib.FIELD_BN254_FQ, to_words([1, 2, 3, 4]))
    grumpkin = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 8, b"not-an-srs")
    short = ctx.bases_upload(_lib.CURVE_BN254_G1, _fixed_mul(ctx, hip, 1, pw[:7]))
    lib.vimz_mlkzg_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32] + hip._MLKZG_TAIL
    out = np.zeros(8 + 4 + 76, dtype=np.uint64)

    def short_cap():
        ctx._chk(lib.vimz_mlkzg_open(ctx.h, srs.h, vec.h, 0, 8, 3, hip._ptr(to_words(point(3))), hip._ptr(out), hip._ptr(out[8:]), hip._ptr(out[12:]), 75, None))

    res["refused"] = {"logn_0": _refusal(lambda: ctx.mlkzg_open(srs, vec, [], n=1)), "logn_27": _refusal(lambda: ctx.mlkzg_open(srs, vec, [1] * 27, n=1)),
                      "n_0": _refusal(lambda: ctx.mlkzg_open(srs, vec, point(3), n=0)), "n_above": _refusal(lambda: ctx.mlkzg_open(srs, vec, point(3), n=9)),
                      "past_the_vector": _refusal(lambda: ctx.mlkzg_open(srs, vec, point(4), n=8, offset=4)),
                      "srs_short": _refusal(lambda: ctx.mlkzg_open(short, vec, point(3), n=7)), "not_fr": _refusal(lambda: ctx.mlkzg_open(srs, fq, point(2))),
                      "not_g1": _refusal(lambda: ctx.mlkzg_open(grumpkin, vec, point(3), n=8)),
                      "point_r": _refusal(lambda: ctx.mlkzg_open(srs, vec, [1, R, 2], n=8)), "cap_short": _refusal(short_cap)}
    res["accepted_after"] = _refusal(lambda: ctx.mlkzg_open(srs, vec, point(3), n=8))
    for h in (vec, fq, grumpkin, short, srs):
        h.free()


def main_cf(ctx, hip, res):
    from tests.test_circuits import step_inputs
    from vimz_amd import _lib
    from vimz_amd.circuit import Circuit
    logn = 16                                                 # the hash step's F': 34.3 k wires and constraints
    srs, vk = hip.kzg_setup(ctx, 1 << logn, seed=b"mlkzg-cf")
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-cyclefold")
    z0, inputs = step_inputs("hash")
    cf = hip.CycleFoldIVC(ctx, Circuit.for_resolution("hash", "HD"), srs, ck2, max_batch=2)
    res["vk"] = hex_of(vk)
    try:
        cf.reset(z0); cf.fold(np.stack(inputs[:3]))
        res["verify"] = cf.verify(3, z0)

        def openings(obj, name):
            Z, E = obj.export(0, hip.IX_RUNNING_Z), obj.export(0, hip.IX_RUNNING_E)
            out = {"instance": hex_of(obj.export(0, hip.IX_INSTANCE)), "Z": hex_of(Z), "E": hex_of(E)}
            for which, n in ((0, len(Z) - 3), (1, len(E))):
                x = point(cf_logn(n), label="cf")
                comm, ev, proof = obj.mlkzg_open(which, x)
                out[str(which)] = {"comm": hex_of(comm), "eval": ev, "proof": hex_of(proof), "verdict": hip.mlkzg_verify(vk, comm, x, ev, proof),
                                   "verdict eval + 1": hip.mlkzg_verify(vk, comm, x, (ev + 1) % R, proof),
                                   "refused": {"logn_above": _refusal(lambda: obj.mlkzg_open(which, x + [1])), "logn_below": _refusal(lambda: obj.mlkzg_open(which, x[:-1]))}}
            res[name] = out

        openings(cf, "cf")
        res["verify_after"] = cf.verify(3, z0)                # (the prover is left as it was)
        cf.reset(z0); cf.fold(np.stack(inputs[:2]))
        m = hip.CycleFoldMerged(cf)
        try:
            res["merged_verify"] = m.verify(2, z0)
            openings(m, "merged")
        finally:
            m.close()
    finally:
        cf.close(); srs.free(); ck2.free()


def run_part(tmp_path_factory, part, timeout=300):
    """what the two test modules do with a part: this script in a child process with the testing library, its JSON read back"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path_factory.mktemp("mlkzg_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._mlkzg_gpu", part, str(out)], cwd=root, capture_output=True, text=True, timeout=timeout,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


def main(part, out_path):
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    res = {"invalid": _lib.ERR_INVALID}
    ctx = hip.Context(0)
    try:
        {"kernels": main_kernels, "open": main_open, "cf": main_cf}[part](ctx, hip, res)
    finally:
        ctx.close()
    with open(out_path, "w") as fp:
        json.dump(res, fp)
    print(f"mlkzg {part} probe ok")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
