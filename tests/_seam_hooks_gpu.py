"""Body of tests/test_gpu_seam_edges.py::test_step_kernels_behind_the_test_hooks, run as a process of its own with VIMZ_HIP_LIBRARY=testing:
k_spmv_cross16 (vimz_test_spmv_cross16) and the boolean-row form of k_cross_term (vimz_test_cross_term_masked) against Python integers.
Test infrastructure."""
import ctypes as C
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CROSS16_FIELDS = (0, 1, 2, 3)
ROW_RANGES = 4                                   # the whole shape; row0 > 0 and a number of rows that is not a multiple of 16; in Montgomery form one row and 30 rows
N_KINDS = 7
N_CROSS16 = len(CROSS16_FIELDS) * (ROW_RANGES * (N_KINDS + N_KINDS * 4) + 1)    # per range: every assignment at step 0 and with a running instance for each of
#                                                                                four u2; then the rows on which the last subtraction needs its whole 3 p
N_MASKED = 4 * 2 * 4                             # four fields, u2 in {1, random}, nb in {0, 1, n - 1, n}
N_IDENTITY = 1


def _u(x):
    import numpy as np
    return np.array([(int(x) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def main():
    from tests import _oracle
    from tests import _seam_cases as sc
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    lib = ctx.lib
    vp = C.c_void_p
    lib.vimz_test_spmv_cross16.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
    lib.vimz_test_cross_term_masked.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_size_t]
    filled = lambda fid, n: ctx.vec_from_host(fid, sc.to_limbs([sc.FILL] * n))
    n_cross16 = n_masked = n_identity = 0
    try:
        # ---- k_spmv_cross16 ---------------------------------------------------------------------------------------------------------------
        for fid in CROSS16_FIELDS:
            p = _lib.MODULUS[fid]
            s = sc.cross16_shape(p, seed=fid)
            assert s.nrows % 16 != 0
            rng = random.Random(f"x16:{fid}")
            run = [[rng.randrange(p) for _ in range(s.nrows)] for _ in range(3)]
            for i in range(0, s.nrows, 5):              # the running instance holds zeros and ones here and there
                run[0][i], run[1][(i + 1) % s.nrows], run[2][(i + 2) % s.nrows] = 0, 1, p - 1
            rund = [ctx.vec_from_host(fid, sc.to_limbs(v)) for v in run]
            u1 = sc.scalars(p, f"{fid}:x16")[3]
            for form in (_lib.FORM_CANONICAL, _lib.FORM_MONTGOMERY):
                mont = form == _lib.FORM_MONTGOMERY
                k = (1 << 256) % p if mont else 1
                S = hip.R1CSShape(ctx, fid, s.nrows, s.ncols, *[s.coo(m, mont=mont) for m in range(3)], form=form)
                ranges = ((0, s.nrows), (3, s.nrows - 3 - 7)) if not mont else ((21, 1), (5, 30))
                for row0, nr in ranges:
                    assert nr == 1 or nr % 16 != 0
                    for kind in sc.Z_KINDS:
                        z = sc.z_vector(kind, p, s.ncols, f"{fid}:x16")
                        want = s.products(z)
                        zd = ctx.vec_from_host(fid, sc.to_limbs(z))
                        for u2 in (None,) + sc.scalars(p, f"{fid}:x16:u2"):          # None: step 0, no running instance
                            outs = [filled(fid, s.nrows + 2) for _ in range(4)]
                            a1 = [v.h if u2 is not None else None for v in rund]
                            ctx._chk(lib.vimz_test_spmv_cross16(ctx.h, S.h, row0, nr, zd.h, outs[0].h, outs[1].h, outs[2].h, a1[0], a1[1], a1[2],
                                                                hip._ptr(_u(u1 * k % p)), hip._ptr(_u((u2 or 0) * k % p)), form, outs[3].h if u2 is not None else None))
                            got = [sc.from_limbs(v.download()) for v in outs]
                            for v in outs:
                                v.free()
                            T = sc.cross_term(p, *run, u1, *want, u2) if u2 is not None else None
                            for m, name in enumerate(("az", "bz", "cz", "T")):
                                ref = (want[m] if m < 3 else T)
                                exp = [sc.FILL] * (s.nrows + 2)
                                if ref is not None:
                                    exp[row0:row0 + nr] = ref[row0:row0 + nr]
                                bad = [i for i in range(len(exp)) if got[m][i] != exp[i]]
                                assert not bad, (f"k_spmv_cross16 field {fid} form {form} rows [{row0}, {row0 + nr}) z {kind} u2 {u2 if u2 is None else hex(u2)} {name}: "
                                                 f"{len(bad)} rows differ, first {bad[0]} ({[s.lens[q][bad[0]] for q in range(3)] if bad[0] < s.nrows else 'beyond nrows'} terms): "
                                                 f"got {got[m][bad[0]]:#x} want {exp[bad[0]]:#x}")
                            n_cross16 += 1
                        zd.free()
                S.free()
            for v in rund:
                v.free()
            # the rows on which T = t1 - t2 + 3 p has t1 = 0 and t2 > 2 p (fresh u = 1)
            s3, z, run, u1 = sc.sub3_limit_case(p, seed=fid)
            S = hip.R1CSShape(ctx, fid, s3.nrows, s3.ncols, *[s3.coo(m) for m in range(3)])
            zd = ctx.vec_from_host(fid, sc.to_limbs(z))
            rund = [ctx.vec_from_host(fid, sc.to_limbs(v)) for v in run]
            outs = [filled(fid, s3.nrows) for _ in range(4)]
            ctx._chk(lib.vimz_test_spmv_cross16(ctx.h, S.h, 0, s3.nrows, zd.h, outs[0].h, outs[1].h, outs[2].h, rund[0].h, rund[1].h, rund[2].h,
                                                hip._ptr(_u(u1)), hip._ptr(_u(1)), _lib.FORM_CANONICAL, outs[3].h))
            got = [sc.from_limbs(v.download()) for v in outs]
            want = s3.products(z)
            want.append(sc.cross_term(p, *run, u1, *want, 1))
            assert want[0] == want[1] == [0] * s3.nrows
            for m, name in enumerate(("az", "bz", "cz", "T")):
                bad = [i for i in range(s3.nrows) if got[m][i] != want[m][i]]
                assert not bad, f"k_spmv_cross16 field {fid} sub<3> limit rows, {name}: {len(bad)} rows differ, first {bad[0]}: got {got[m][bad[0]]:#x} want {want[m][bad[0]]:#x}"
            for v in outs + rund + [zd]:
                v.free()
            S.free()
            n_cross16 += 1
        # ---- k_cross_term with the boolean-row vector --------------------------------------------------------------------------------------
        n = 3001
        for fid in (0, 1, 2, 3):
            p = _lib.MODULUS[fid]
            rng = random.Random(f"masked:{fid}")
            fresh = lambda: [(0, 1, 0, 1, p - 1, 2, rng.randrange(p))[rng.randrange(7)] for _ in range(n)]
            v1 = [[rng.randrange(p) for _ in range(n)] for _ in range(3)]
            v2 = [fresh() for _ in range(3)]
            for i in range(64, 192):                    # whole waves of one class
                v2[0][i] = 1 if i < 128 else 0
            for i in range(192, 256):
                v2[0][i] = rng.randrange(2, p)         # a wave in which no fresh az is boolean
            d1 = [ctx.vec_from_host(fid, sc.to_limbs(v)) for v in v1]
            d2 = [ctx.vec_from_host(fid, sc.to_limbs(v)) for v in v2]
            u1 = sc.scalars(p, f"{fid}:masked")[3]
            for u2 in (1, sc.scalars(p, f"{fid}:masked:u2")[3]):
                T = sc.cross_term(p, *v1, u1, *v2, u2)
                Tplain = filled(fid, n + 2)
                ctx._chk(lib.vimz_test_cross_term_masked(ctx.h, n, d1[0].h, d1[1].h, d1[2].h, hip._ptr(_u(u1)), d2[0].h, d2[1].h, d2[2].h, hip._ptr(_u(u2)), _lib.FORM_CANONICAL, Tplain.h, None, 0))
                plain = sc.from_limbs(Tplain.download()); Tplain.free()
                assert plain == T + [sc.FILL] * 2, f"k_cross_term field {fid} u2 {u2:#x}: T without the boolean-row vector"
                for nb in (0, 1, n - 1, n):
                    Td, Tm = filled(fid, n + 2), filled(fid, n + 2)
                    ctx._chk(lib.vimz_test_cross_term_masked(ctx.h, n, d1[0].h, d1[1].h, d1[2].h, hip._ptr(_u(u1)), d2[0].h, d2[1].h, d2[2].h, hip._ptr(_u(u2)), _lib.FORM_CANONICAL, Td.h, Tm.h, nb))
                    got, gotm = sc.from_limbs(Td.download()), sc.from_limbs(Tm.download())
                    Td.free(); Tm.free()
                    assert got == plain, f"k_cross_term field {fid} u2 {u2:#x} nb {nb}: T changed by the presence of Tm"
                    want = [(2 * T[i] % p if v2[0][i] == 1 else 0 if v2[0][i] == 0 else (T[i] + v1[0][i]) % p) if i < nb else T[i] for i in range(n)] + [sc.FILL] * 2
                    bad = [i for i in range(n + 2) if gotm[i] != want[i]]
                    assert not bad, (f"k_cross_term field {fid} u2 {u2:#x} nb {nb}: Tm differs on {len(bad)} rows, first {bad[0]} (fresh az {v2[0][bad[0]] if bad[0] < n else None}): "
                                     f"got {gotm[bad[0]]:#x} want {want[bad[0]]:#x}")
                    n_masked += 1
            for v in d1 + d2:
                v.free()
        # ---- the identity the IVC relies on (r1cs_ops.hpp, "The BOOLEAN-ROW form"), with the oracle's curve arithmetic -------------------------
        #   sum_{i<nb} T_i ck_i = sum_{i<nb} Tm_i ck_i + u1 S_1 - C_A,  S_1 = sum_{fresh az_i = 1} ck_i,  C_A = sum_{i<nb} az1_i ck_i
        # on rows b (b - 1) = 0 of a running instance (az1 = a, bz1 = a - u1, cz1 = 0) and a fresh one (az2 = b, bz2 = b - 1, cz2 = 0, u2 = 1) whose b is
        # NOT always boolean: such a row gets T_i + a_i.
        oracle = _oracle.load()
        fid, curve = 0, 0
        p = _lib.MODULUS[fid]
        n, nb = 2500, 2100
        rng = random.Random("identity")
        u1 = rng.randrange(2, p)
        a = [rng.randrange(p) for _ in range(n)]
        b = [(0, 1, 0, 1, 0, 1, 0, 1, 7, rng.randrange(2, p))[rng.randrange(10)] for _ in range(n)]
        assert sum(1 for x in b[:nb] if x > 1) > 100
        v1 = [a, [(x - u1) % p for x in a], [0] * n]
        v2 = [b, [(x - 1) % p for x in b], [0] * n]
        for i in range(nb, n):                          # the rows behind the boolean ones are ordinary
            v1[1][i], v1[2][i], v2[1][i], v2[2][i] = rng.randrange(p), rng.randrange(p), rng.randrange(p), rng.randrange(p)
        d1 = [ctx.vec_from_host(fid, sc.to_limbs(v)) for v in v1]
        d2 = [ctx.vec_from_host(fid, sc.to_limbs(v)) for v in v2]
        Td, Tm = filled(fid, n), filled(fid, n)
        ctx._chk(lib.vimz_test_cross_term_masked(ctx.h, n, d1[0].h, d1[1].h, d1[2].h, hip._ptr(_u(u1)), d2[0].h, d2[1].h, d2[2].h, hip._ptr(_u(1)), _lib.FORM_CANONICAL, Td.h, Tm.h, nb))
        T, M = Td.download(), Tm.download()
        for v in d1 + d2 + [Td, Tm]:
            v.free()
        assert sc.from_limbs(T) == sc.cross_term(p, *v1, u1, *v2, 1)
        ck = oracle.seq_bases(curve, n)
        ones = [i for i in range(nb) if b[i] == 1]
        S1 = oracle.msm(curve, ck[ones], sc.to_limbs([1] * len(ones)))
        CA = oracle.msm(curve, ck[:nb], sc.to_limbs(a[:nb]))
        lhs = oracle.msm(curve, ck[:nb], T[:nb])
        rhs = oracle.curve_add(curve, oracle.curve_add(curve, oracle.msm(curve, ck[:nb], M[:nb]), oracle.curve_mul(curve, S1, u1)), oracle.curve_mul(curve, CA, p - 1))
        assert lhs == rhs and lhs != (0, 0), "boolean-row identity: sum T_i ck_i != sum Tm_i ck_i + u1 S_1 - C_A"
        assert oracle.msm(curve, ck, T) == oracle.curve_add(curve, rhs, oracle.msm(curve, ck[nb:], M[nb:]))          # and the other rows are T itself
        n_identity += 1
    finally:
        ctx.close()
    assert len(sc.Z_KINDS) == N_KINDS
    assert (n_cross16, n_masked, n_identity) == (N_CROSS16, N_MASKED, N_IDENTITY), (n_cross16, n_masked, n_identity)
    print(f"seam hooks ok: cross16 {n_cross16} masked {n_masked} identity {n_identity}")


if __name__ == "__main__":
    main()
