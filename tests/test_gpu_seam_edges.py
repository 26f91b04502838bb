"""The SpMV / cross-term seam at the shapes and values where its kernels branch (tests/_seam_cases.py): rows at the boundaries of the one-thread /
sixteen-lane / wave paths (with the classes laid out by wave step: tests/_seam_cases.py), a 70 000-term row (34 reductions inside a lane), empty rows and matrices, duplicate triplets, zero coefficients; assignments
that are all 0, all 1, all p - 1, random, witness-like and a lane-by-lane cross of value and coefficient classes; outputs pre-filled and compared over
their whole length.  Reference: Python integers; the oracle's spmv / cross_term as a second opinion (checked without a GPU too)."""
import os
import subprocess
import sys

import pytest

from tests import _seam_cases as sc
from vimz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [_lib.FIELD_BN254_FR, _lib.FIELD_BN254_FQ, _lib.FIELD_PALLAS_FP, _lib.FIELD_VESTA_FQ]
CURVE_OF_SCALAR_FIELD = {f: c for c, f in _lib.CURVE_SCALAR_FIELD.items()}
FORMS = (_lib.FORM_CANONICAL, _lib.FORM_MONTGOMERY)
N_SHAPES = 13
_cache = {}


def _shapes(fid):
    if ("shapes", fid) not in _cache:
        _cache["shapes", fid] = sc.shapes(_lib.MODULUS[fid], seed=fid)
    return _cache["shapes", fid]


def _z(fid, shape, kind):
    key = ("z", fid, shape.name, kind)
    if key not in _cache:
        _cache[key] = sc.z_vector(kind, shape.p, shape.ncols, f"{fid}:{shape.name}")
    return _cache[key]


def _products(fid, shape, kind):
    key = ("prod", fid, shape.name, kind)
    if key not in _cache:
        _cache[key] = shape.products(_z(fid, shape, kind))
    return _cache[key]


def _in_form(vals, p, form):
    return sc.to_limbs(vals if form == _lib.FORM_CANONICAL else [v * (1 << 256) % p for v in vals])


def _scalar_in_form(u, p, form):
    return u if form == _lib.FORM_CANONICAL else u * (1 << 256) % p


@pytest.fixture(scope="module")
def ctx():
    from vimz_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("fid", FIELDS)
def test_cases_and_integer_reference_agree_with_the_oracle(oracle, fid):
    """No GPU: every shape and assignment of the generator through the Python-integer reference and through the oracle's spmv / cross_term."""
    p = _lib.MODULUS[fid]
    assert oracle.modulus[fid] == p
    shapes = _shapes(fid)
    assert len(shapes) == N_SHAPES
    ran = 0
    for s in shapes:
        info = s.expect_info()
        assert info["n_long"] == sum(1 for m in range(3) for k in s.lens[m] if k > sc.SPMV_LONG)
        csr = [s.csr(m) for m in range(3)]
        prods = {}
        for kind in sc.Z_KINDS:
            z = _z(fid, s, kind)
            want = _products(fid, s, kind)
            for m in range(3):
                got = oracle.spmv(fid, s.nrows, s.ncols, *csr[m], sc.to_limbs(z))
                assert sc.from_limbs(got) == want[m], f"field {fid} shape {s.name} z {kind} matrix {m}: reference and oracle differ"
                ran += 1
            prods[kind] = want
        for u1 in sc.scalars(p, f"{fid}:u1"):
            for u2 in sc.scalars(p, f"{fid}:u2"):
                want = sc.cross_term(p, *prods["random"], u1, *prods["witness"], u2)
                got = oracle.cross_term(fid, *[sc.to_limbs(v) for v in prods["random"]], u1, *[sc.to_limbs(v) for v in prods["witness"]], u2)
                assert sc.from_limbs(got) == want, f"field {fid} shape {s.name}: cross term u1 {u1:#x} u2 {u2:#x}"
                ran += 1
    assert ran == N_SHAPES * (3 * len(sc.Z_KINDS) + 16)
    st = shapes[0]
    n = len(sc.STAGGER)
    assert st.name == "staggered" and all(st.lens[m][:n] == [sc.STAGGER[(i + 7 * m) % n] for i in range(n)] for m in range(3))      # every count, in every matrix
    assert {k % 4 for k in (s.expect_info()["n_med"] for s in shapes if "nmed" in s.name)} == {0, 1, 2, 3}
    # the shapes behind the hooks and the relaxed check, validated here as well
    x16 = sc.cross16_shape(p, seed=fid)
    sat, base = sc.sat_shape(p, seed=fid)
    zsat = sc.satisfy(sat, base, sc.z_vector("witness", p, base, f"{fid}:sat"), 3)
    for s, z in ((x16, sc.z_vector("cross", p, x16.ncols, f"{fid}:x16")), (sat, zsat)):
        for m in range(3):
            assert sc.from_limbs(oracle.spmv(fid, s.nrows, s.ncols, *s.csr(m), sc.to_limbs(z))) == s.spmv(m, z), f"field {fid} shape {s.name} matrix {m}"
    assert oracle.first_unsat(fid, *[sc.to_limbs(v) for v in sat.products(zsat)], u=3) == -1
    s3, z3, run3, u13 = sc.sub3_limit_case(p, seed=fid)
    assert s3.nrows == 21 and len(z3) == 21 and s3.lens == [[0] * 21, [0] * 21, [1] * 21] and run3[2] == [(p - 1) * pow(1 << 256, -1, p) % p] * 21
    # The layout the ballots are meant to see (tests/_seam_cases.py: wave_step), counted on the term order the upload produces: by construction a third
    # of the wave steps is uniform in one (value, coefficient) pair and a third holds every pair lane by lane; partly filled steps leave at least a
    # quarter of each, and the uniform steps of a path cover every coefficient class and every value class.
    for s, path in ((st, "thread"), (st, "wave"), (next(s for s in shapes if s.name == "quads"), "quad"), (x16, "cross16")):
        c = sc.wave_census(s)[path]
        assert c["steps"] >= 90 and 4 * c["uniform"] >= c["steps"] and 4 * c["every_class"] >= c["steps"], (fid, s.name, path, c)
        assert {a for a, _ in c["uniform_pairs"]} == set(range(5)) and {b for _, b in c["uniform_pairs"]} == set(range(5)), (fid, s.name, path, c["uniform_pairs"])
    assert sc.wave_census(next(s for s in shapes if s.name == "shuffled"))["thread"]["steps"] >= 60          # (fully shuffled: no layout to speak of)


def _filled(ctx, fid, n):
    return ctx.vec_from_host(fid, sc.to_limbs([sc.FILL] * n))


@pytest.mark.gpu
@pytest.mark.parametrize("fid", FIELDS)
def test_multiply_vec_at_the_edges(ctx, fid):
    """vimz_r1cs_upload / vimz_r1cs_info / vimz_spmv3: every shape in both upload forms, every assignment, into pre-filled vectors three elements longer
    than the shape (what lies beyond nrows keeps the fill)."""
    from vimz_amd import hip
    p = _lib.MODULUS[fid]
    ran = 0
    for s in _shapes(fid):
        for form in FORMS:
            S = hip.R1CSShape(ctx, fid, s.nrows, s.ncols, *[s.coo(m, mont=form == _lib.FORM_MONTGOMERY) for m in range(3)], form=form)
            try:
                info, want_info = S.info(), s.expect_info()
                assert {k: info[k] for k in want_info if k != "n_med"} == {k: v for k, v in want_info.items() if k != "n_med"} and info["field"] == fid, (fid, s.name, info, want_info)
                for kind in sc.Z_KINDS:
                    zd = ctx.vec_from_host(fid, _in_form(_z(fid, s, kind), p, form), form=form)
                    outs = [_filled(ctx, fid, s.nrows + 3) for _ in range(3)]
                    try:
                        S.multiply_vec(zd, out=outs)
                        want = _products(fid, s, kind)
                        for m in range(3):
                            got = sc.from_limbs(outs[m].download())
                            bad = [i for i in range(s.nrows) if got[i] != want[m][i]]
                            assert not bad, (f"field {fid} shape {s.name} form {form} z {kind} matrix {'ABC'[m]}: {len(bad)} rows differ, first row {bad[0]} "
                                             f"({s.lens[m][bad[0]]} terms): got {got[bad[0]]:#x} want {want[m][bad[0]]:#x}")
                            assert got[s.nrows:] == [sc.FILL] * 3, f"field {fid} shape {s.name} matrix {'ABC'[m]}: written beyond nrows"
                        ran += 1
                    finally:
                        for v in outs + [zd]:
                            v.free()
            finally:
                S.free()
    assert ran == N_SHAPES * 2 * len(sc.Z_KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("fid", FIELDS)
def test_commit_T_at_the_edges(ctx, oracle, fid):
    """vimz_commit_T with u1 and u2 each in {0, 1, p - 1, random}, a witness-like and a dense fresh assignment, both forms, T pre-filled: T against Python
    integers, its commitment against the oracle's MSM of the reference T."""
    from vimz_amd import hip
    p = _lib.MODULUS[fid]
    curve = CURVE_OF_SCALAR_FIELD[fid]
    s = _shapes(fid)[0]
    bases = oracle.seq_bases(curve, s.nrows)
    ck = ctx.bases_upload(curve, bases)
    Ss = [hip.R1CSShape(ctx, fid, s.nrows, s.ncols, *[s.coo(m, mont=form == _lib.FORM_MONTGOMERY) for m in range(3)], form=form) for form in FORMS]
    z1 = ctx.vec_from_host(fid, sc.to_limbs(_z(fid, s, "random")))
    p1 = _products(fid, s, "random")
    ran = 0
    try:
        for kind in ("witness", "cross"):              # mostly 0 / 1, and dense in every class
            z2 = ctx.vec_from_host(fid, sc.to_limbs(_z(fid, s, kind)))
            p2 = _products(fid, s, kind)
            for i, u1 in enumerate(sc.scalars(p, f"{fid}:u1")):
                for j, u2 in enumerate(sc.scalars(p, f"{fid}:u2")):
                    form = FORMS[(i + j) & 1]
                    T = _filled(ctx, fid, s.nrows + 3)
                    try:
                        _, comm = Ss[form].commit_T(ck, z1, _scalar_in_form(u1, p, form), z2, _scalar_in_form(u2, p, form), out=T, form=form)
                        want = sc.cross_term(p, *p1, u1, *p2, u2)
                        got = sc.from_limbs(T.download())
                        bad = [r for r in range(s.nrows) if got[r] != want[r]]
                        assert not bad, f"field {fid} z2 {kind} u1 {u1:#x} u2 {u2:#x} form {form}: T differs on {len(bad)} rows, first {bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"
                        assert got[s.nrows:] == [sc.FILL] * 3, "T written beyond nrows"
                        assert tuple(sc.from_limbs(comm)) == oracle.msm(curve, bases, sc.to_limbs(want), threads=8), f"field {fid} z2 {kind} u1 {u1:#x} u2 {u2:#x}: comm_T"
                        ran += 1
                    finally:
                        T.free()
            z2.free()
    finally:
        z1.free(); ck.free()
        for S in Ss:
            S.free()
    assert ran == 32


@pytest.mark.gpu
@pytest.mark.parametrize("fid", FIELDS)
def test_check_relaxed_counts_and_finds_the_first_bad_row(ctx, fid):
    """vimz_r1cs_check_relaxed: a satisfied assignment (0 rows, no first), one bad row at 0, nrows - 1, 255, 256, several bad rows (count and minimum),
    with and without an error vector, and u = 0."""
    from vimz_amd import hip
    p = _lib.MODULUS[fid]
    s, base = sc.sat_shape(p, seed=fid)
    S = hip.R1CSShape(ctx, fid, s.nrows, s.ncols, *[s.coo(m) for m in range(3)])
    u = sc.scalars(p, f"{fid}:relaxed")[3]
    free = sc.z_vector("witness", p, base, f"{fid}:sat")
    ran = 0
    try:
        for uu in (1, u):
            z = sc.satisfy(s, base, free, uu)
            az, bz, cz = s.products(z)
            assert sc.unsat_rows(p, az, bz, cz, uu) == []
            E = [0] * s.nrows
            for bad_rows in ([], [0], [s.nrows - 1], [255], [256], [256, 17, 255, s.nrows - 1], list(range(s.nrows))):
                for with_E in (False, True):
                    zz, EE = list(z), list(E)
                    for r in bad_rows:
                        if with_E and r % 2:
                            EE[r] = (EE[r] + 1) % p                      # the error vector is what is wrong
                        else:
                            zz[base + r] = (zz[base + r] + 1) % p       # cz_r is
                    zd = ctx.vec_from_host(fid, sc.to_limbs(zz))
                    Ed = ctx.vec_from_host(fid, sc.to_limbs(EE)) if with_E else None
                    try:
                        got = S.check_relaxed(zd, uu, Ed)
                    finally:
                        zd.free()
                        if Ed is not None:
                            Ed.free()
                    want = sc.unsat_rows(p, *s.products(zz), uu, EE if with_E else None)
                    assert want == sorted(bad_rows)
                    assert got == (len(want), min(want) if want else None), f"field {fid} u {uu:#x} bad rows {bad_rows} E {with_E}: got {got}"
                    ran += 1
        # a relaxed instance proper: a dense error vector E = az∘bz - u·cz for an arbitrary assignment, and u = 0 (E = az∘bz)
        for uu in (u, 0):
            z = sc.z_vector("random", p, s.ncols, f"{fid}:relaxed:{uu}")
            az, bz, cz = s.products(z)
            E = [(a * b - uu * c) % p for a, b, c in zip(az, bz, cz)]
            for bad_rows in ([], [0, 256]):
                EE = list(E)
                for r in bad_rows:
                    EE[r] = (EE[r] + p - 1) % p
                zd, Ed = ctx.vec_from_host(fid, sc.to_limbs(z)), ctx.vec_from_host(fid, sc.to_limbs(EE))
                try:
                    got = S.check_relaxed(zd, uu, Ed)
                finally:
                    zd.free(); Ed.free()
                assert got == (len(bad_rows), min(bad_rows) if bad_rows else None), f"field {fid} u {uu:#x} dense E, bad rows {bad_rows}: got {got}"
                ran += 1
    finally:
        S.free()
    assert ran == 2 * 7 * 2 + 4


@pytest.mark.gpu
@pytest.mark.parametrize("fid", FIELDS)
def test_vec_axpy_at_the_edges(ctx, fid):
    """vimz_vec_axpy for n in {0, 1, 255, 256, 257, 2048·256 + 3} (the last makes the stride loop's second pass) and r in {0, 1, p - 1, random}, both
    forms of r; what lies beyond n is untouched."""
    from vimz_amd import hip
    import random
    p = _lib.MODULUS[fid]
    big = 2048 * 256 + 3
    rng = random.Random(f"axpy:{fid}")
    a = [rng.randrange(p) for _ in range(big + 5)]
    b = [rng.randrange(p) for _ in range(big + 5)]
    for i in range(0, big, 1000):                      # the classes a fresh vector is made of, here and there
        b[i], b[i + 1], b[i + 2], a[i + 3] = 0, 1, p - 1, 0
    x2 = ctx.vec_from_host(fid, sc.to_limbs(b))
    ran = 0
    try:
        for n in (0, 1, 255, 256, 257, big):
            total = n + 5
            for k, r in enumerate(sc.scalars(p, f"{fid}:axpy")):
                form = FORMS[k & 1]
                x1 = ctx.vec_from_host(fid, sc.to_limbs(a[:total]))
                try:
                    hip.vec_axpy(ctx, x1, _scalar_in_form(r, p, form), x2, n=n, form=form)
                    got = sc.from_limbs(x1.download())
                finally:
                    x1.free()
                want = [(x + r * y) % p for x, y in zip(a[:n], b[:n])] + a[n:total]
                bad = [i for i in range(total) if got[i] != want[i]]
                assert not bad, f"field {fid} n {n} r {r:#x} form {form}: {len(bad)} elements differ, first {bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"
                ran += 1
    finally:
        x2.free()
    assert ran == 24


@pytest.mark.gpu
def test_step_kernels_behind_the_test_hooks():
    """k_spmv_cross16 and the boolean-row form of k_cross_term (vimz_test_spmv_cross16, vimz_test_cross_term_masked: hooks of libvimz_hip_testing.so
    only) against Python integers, and the identity the IVC's commitment of a boolean-row cross term relies on against the oracle's curve
    arithmetic.  The body (tests/_seam_hooks_gpu.py) runs in a process of its own on the testing library."""
    env = dict(os.environ, VIMZ_HIP_LIBRARY="testing")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_seam_hooks_gpu.py")], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from tests import _seam_hooks_gpu as body
    assert f"seam hooks ok: cross16 {body.N_CROSS16} masked {body.N_MASKED} identity {body.N_IDENTITY}" in r.stdout, r.stdout[-2000:]
