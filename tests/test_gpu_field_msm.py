"""GPU parity: device Montgomery arithmetic, XYZZ group law and the Pippenger MSM pipeline, each called
through the C ABI (include/vimz_hip.h) and compared bit-for-bit with the CPU oracle."""
import random

import numpy as np
import pytest

from tests._oracle import CURVE_BASE, CURVE_SCALAR, GENERATORS, from_limbs, to_limbs
from vimz_amd import _lib

pytestmark = pytest.mark.gpu

MODULI = {
    0: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
    1: 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47,
    2: 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
    3: 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
}


@pytest.fixture(scope="module")
def ctx():
    from vimz_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def rand_scalars(rng, n, mod):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in (rng.randrange(mod) for _ in range(n))], dtype=np.uint64)


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_field_ops_match_oracle(ctx, oracle, fid):
    p = MODULI[fid]
    rng = random.Random(100 + fid)
    edge = [0, 1, 2, p - 1, p - 2, (1 << 255) % p, (1 << 128) - 1, (1 << 32) - 1, 1 << 32, (1 << 224)]
    a = edge + [rng.randrange(p) for _ in range(2000)]
    b = list(reversed(edge)) + [rng.randrange(p) for _ in range(2000)]
    A, B = to_limbs(a), to_limbs(b)
    assert from_limbs(ctx.field_op(fid, "add", A, B)) == [(x + y) % p for x, y in zip(a, b)]
    assert from_limbs(ctx.field_op(fid, "sub", A, B)) == [(x - y) % p for x, y in zip(a, b)]
    got = from_limbs(ctx.field_op(fid, "mul", A, B))
    assert got == [(x * y) % p for x, y in zip(a, b)]
    # and against the oracle's own Montgomery implementation on a sample
    for i in range(0, 60):
        assert got[i] == oracle.f_mul(fid, a[i], b[i])
    inv = from_limbs(ctx.field_op(fid, "inv", A[:64]))
    assert inv == [pow(x, p - 2, p) for x in a[:64]]


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_field_ops_on_limb_patterns_match_python_integers(ctx, fid):
    """The 8 x 32 Montgomery field on the device (vimz_field_op) on operands whose 32-bit limbs all come from {0, 1, 0x7fffffff, 0x80000000, 0xffffffff}
    (reduced below p by clearing top bits): uniform, alternating, one limb different, random draws — the carry and borrow chains random operands
    never build — for add / sub / mul / inv against Python integers."""
    from tests._fp29_ref import word_patterns
    p = MODULI[fid]
    rng = random.Random(700 + fid)
    pats = word_patterns(rng, p, n_random=1000)
    assert len(pats) >= 1100 and all(0 <= x < p for x in pats) and {0, 1} <= set(pats)
    a = pats + [pats[(7 * i + 3) % len(pats)] for i in range(len(pats))] + pats
    b = pats[::-1] + pats + [rng.randrange(p) for _ in pats]
    A, B = to_limbs(a), to_limbs(b)
    for op, fn in (("add", lambda x, y: (x + y) % p), ("sub", lambda x, y: (x - y) % p), ("mul", lambda x, y: x * y % p)):
        got = from_limbs(ctx.field_op(fid, op, A, B))
        bad = [i for i in range(len(a)) if got[i] != fn(a[i], b[i])]
        assert not bad, f"field {fid} {op}: {len(bad)} of {len(a)} differ, first a = {a[bad[0]]:#x} b = {b[bad[0]]:#x} got {got[bad[0]]:#x}"
    inv = from_limbs(ctx.field_op(fid, "inv", to_limbs(pats)))
    bad = [i for i, x in enumerate(pats) if inv[i] != pow(x, p - 2, p)]
    assert not bad, f"field {fid} inv: {len(bad)} of {len(pats)} differ, first a = {pats[bad[0]]:#x} got {inv[bad[0]]:#x}"


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_group_law_matches_oracle(ctx, oracle, cid):
    r = MODULI[CURVE_SCALAR[cid]]
    G = GENERATORS[cid]
    rng = random.Random(cid)
    ks = [rng.randrange(r) for _ in range(24)]
    pts = [oracle.curve_mul(cid, G, k) for k in ks]
    P = pts[:12] + [pts[0], pts[1], (0, 0), pts[2], (0, 0)]
    negp1 = oracle.curve_mul(cid, G, r - ks[1])
    Q = pts[12:] + [pts[0], negp1, pts[3], (0, 0), (0, 0)]          # doubling, cancellation, identities
    got = ctx.curve_add(cid, np.array([to_limbs(p).reshape(-1) for p in P]), np.array([to_limbs(q).reshape(-1) for q in Q]))
    want = [oracle.curve_add(cid, p, q) for p, q in zip(P, Q)]
    assert [tuple(from_limbs(g)) for g in got] == want
    assert want[13] == (0, 0)


def _msm_case(ctx, oracle, cid, n, scal_ints, bases=None, window_bits=0, mont=False):
    from vimz_amd import _lib
    if bases is None:
        bases = oracle.seq_bases(cid, n)
    S = to_limbs(scal_ints)
    want = oracle.msm(cid, bases, S, threads=8)
    B = ctx.bases_upload(cid, bases)
    try:
        if mont:
            Sm = oracle.to_mont(CURVE_SCALAR[cid], S)
            got = ctx.msm(B, Sm, form=_lib.FORM_MONTGOMERY, window_bits=window_bits)
        else:
            got = ctx.msm(B, S, window_bits=window_bits)
    finally:
        B.free()
    assert tuple(from_limbs(got)) == want
    return want


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 33, 1000])
def test_msm_small_all_curves(ctx, oracle, cid, n):
    r = MODULI[CURVE_SCALAR[cid]]
    rng = random.Random(n * 10 + cid)
    sc = [rng.randrange(r) for _ in range(n)]
    _msm_case(ctx, oracle, cid, n, sc)


@pytest.mark.parametrize("n", [1535, 1536, 1537, 7709, 24576, 24577, 30720, 30721])
@pytest.mark.parametrize("kind", ["dense", "witness"])
def test_msm_around_the_fused_kernel_boundaries(ctx, oracle, n, kind):
    """Sizes at the edges of the single-launch small MSM (1536 points per workgroup chunk, 30 720 points — twenty chunks — in all; 24 576 was the limit until round 3) and just past
    it (general pipeline with short sub-buckets), for dense scalars and for witness-like ones (mostly 0/1 and bytes)."""
    r = MODULI[CURVE_SCALAR[1]]
    rng = random.Random(f"{n}-{kind}")
    if kind == "dense":
        sc = [rng.randrange(r) for _ in range(n)]
    else:
        sc = [rng.choice([0, 1, 1, 1, rng.randrange(256), rng.randrange(r)]) for _ in range(n)]
        sc[-1] = r - 1
    _msm_case(ctx, oracle, 1, n, sc)


def test_msm_empty(ctx, oracle):
    B = ctx.bases_upload(0, oracle.seq_bases(0, 4))
    assert tuple(from_limbs(ctx.msm(B, np.zeros((0, 4), dtype=np.uint64)))) == (0, 0)
    B.free()


@pytest.mark.parametrize("c", [4, 7, 10, 13, 16])
def test_msm_window_sizes(ctx, oracle, c):
    r = MODULI[0]
    rng = random.Random(c)
    n = 3000
    _msm_case(ctx, oracle, 0, n, [rng.randrange(r) for _ in range(n)], window_bits=c)


def test_msm_edge_scalars(ctx, oracle):
    r = MODULI[0]
    n = 2048
    rng = random.Random(5)
    sc = [0, 1, r - 1, r - 2, 2, (1 << 253), (1 << 128) - 1, (1 << 64), 255, 256] * 8
    sc += [rng.randrange(r) for _ in range(n - len(sc))]
    _msm_case(ctx, oracle, 0, n, sc)
    _msm_case(ctx, oracle, 0, n, [0] * n)
    _msm_case(ctx, oracle, 0, n, [r - 1] * n)
    _msm_case(ctx, oracle, 0, n, [1] * n)


def test_msm_repeated_and_identity_bases(ctx, oracle):
    """All bases equal (forces the doubling branch inside bucket accumulation) + identity bases."""
    n = 4096
    G = to_limbs(GENERATORS[0]).reshape(1, 8)
    bases = np.tile(G, (n, 1))
    bases[7] = 0
    bases[100:110] = 0
    rng = random.Random(9)
    sc = [rng.randrange(1 << 20) for _ in range(n)]
    sc[:64] = [3] * 64
    got = _msm_case(ctx, oracle, 0, n, sc, bases=bases)
    k = sum(s for i, s in enumerate(sc) if i != 7 and not (100 <= i < 110)) % MODULI[0]
    assert got == oracle.curve_mul(0, GENERATORS[0], k)
    # P and -P in the same bucket: cancellation inside a bucket
    negG = oracle.curve_mul(0, GENERATORS[0], MODULI[0] - 1)
    bases2 = np.tile(G, (64, 1))
    bases2[1::2] = to_limbs(negG).reshape(1, 8)
    assert _msm_case(ctx, oracle, 0, 64, [5] * 64, bases=bases2) == (0, 0)


def test_msm_witness_like_scalars(ctx, oracle):
    """~95 % bits/bytes, 5 % full-width: one bucket holds a third of all points -> sub-bucket split + combine."""
    r = MODULI[0]
    n = 60000
    rng = random.Random(11)
    sc = []
    for i in range(n):
        u = rng.random()
        sc.append(rng.randrange(2) if u < 0.8 else rng.randrange(256) if u < 0.95 else rng.randrange(r))
    _msm_case(ctx, oracle, 0, n, sc)


def test_msm_split_ones_path(ctx, oracle):
    """Unit scalars summed by the dedicated tree kernel: same result as the oracle, for witness-like and edge inputs."""
    from vimz_amd import _lib
    r = MODULI[0]
    rng = random.Random(17)
    # (the units are compacted through a per-wave LDS queue, 64 at a time — k_ones_dense: sizes that are no multiple of 64, queues that
    #  never fill, a lone unit in the last partial block, a lane that meets the same base twice)
    for n, mk in ((1, lambda: 1), (64, lambda: 1), (40000, lambda: rng.choice([0, 1, 1, 1, rng.randrange(256), rng.randrange(r)])), (3000, lambda: 0),
                  (4133, lambda: 1), (70001, lambda: 1 if rng.random() < 0.4 else rng.randrange(1 << 16)), (129, None), (128, lambda: 1)):
        sc = [mk() for _ in range(n)] if mk else [0] * 128 + [1]
        bases = oracle.seq_bases(0, n)
        if n == 128:
            bases[:] = to_limbs(GENERATORS[0]).reshape(1, 8)         # every base the same: a lane adds P to P
        if n == 64:
            bases[::2] = to_limbs(GENERATORS[0]).reshape(1, 8)       # repeated bases: doubling inside the ones tree
            bases[1::2] = to_limbs(oracle.curve_mul(0, GENERATORS[0], r - 1)).reshape(1, 8)   # and cancellation
        want = oracle.msm(0, bases, to_limbs(sc), threads=8)
        B = ctx.bases_upload(0, bases)
        v = ctx.vec_from_host(_lib.FIELD_BN254_FR, to_limbs(sc))
        try:
            assert tuple(from_limbs(ctx.msm_vec(B, v, split_ones=True))) == want
            assert tuple(from_limbs(ctx.msm_vec(B, v, split_ones=False))) == want
        finally:
            v.free(); B.free()


def test_msm_montgomery_scalars_and_resident_vectors(ctx, oracle):
    from vimz_amd import _lib
    r = MODULI[0]
    n = 5000
    rng = random.Random(13)
    sc = [rng.randrange(r) for _ in range(n)]
    want = _msm_case(ctx, oracle, 0, n, sc, mont=True)
    bases = oracle.seq_bases(0, n)
    B = ctx.bases_upload(0, oracle.to_mont(CURVE_BASE[0], bases.reshape(-1, 4)).reshape(-1, 8), form=_lib.FORM_MONTGOMERY)
    v = ctx.vec_from_host(_lib.FIELD_BN254_FR, to_limbs(sc))
    assert tuple(from_limbs(ctx.msm_vec(B, v))) == want
    assert from_limbs(v.download()) == sc
    # sub-range against a base offset: sum_{i in [100,600)} s_i * P_i
    sub = oracle.msm(0, bases[100:600], to_limbs(sc[100:600]))
    assert tuple(from_limbs(ctx.msm_vec(B, v, n=500, offset=100, base_offset=100))) == sub
    v.free(); B.free()


def test_msm_large_dense(ctx, oracle):
    """n = 2^17 uniform 254-bit scalars (the MSM(T) shape); linearity check at full size."""
    r = MODULI[0]
    n = 1 << 17
    rs = np.random.default_rng(1)
    raw = rs.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    raw[:, 3] &= np.uint64((1 << 60) - 1)       # < 2^252 < r
    bases = oracle.seq_bases(0, n)
    want = oracle.msm(0, bases, raw, threads=8)
    B = ctx.bases_upload(0, bases)
    got = tuple(from_limbs(ctx.msm(B, raw)))
    assert got == want
    # linearity: MSM(s) + MSM(s') == MSM(s + s')  (size-independent property)
    raw2 = rs.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    raw2[:, 3] &= np.uint64((1 << 60) - 1)
    s1, s2 = from_limbs(raw), from_limbs(raw2)
    ssum = to_limbs([(a + b) % r for a, b in zip(s1, s2)])
    g2 = tuple(from_limbs(ctx.msm(B, raw2)))
    g3 = tuple(from_limbs(ctx.msm(B, ssum)))
    assert oracle.curve_add(0, got, g2) == g3
    B.free()


def test_msm_2_19_dense_and_real_error_vector(ctx, oracle):
    """The headline launches are 305 k / 313 k points over a 2^19 key: oracle parity at n = 2^19 on (a) uniform 254-bit scalars and
    (b) a REAL running error vector E exported from a contrast-HD IVC after eight folds (41 % zeros, repeated values, heavy
    buckets — the structure DESIGN.md §9 describes), zero-padded to 2^19."""
    from tests.test_circuits import step_inputs
    from vimz_amd import hip
    from vimz_amd.circuit import Circuit
    n = 1 << 19
    rs = np.random.default_rng(19)
    raw = rs.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    raw[:, 3] &= np.uint64((1 << 60) - 1)
    ck = ctx.bases_generate(_lib.CURVE_BN254_G1, n)
    bases = ck.download(0, n)
    assert tuple(from_limbs(ctx.msm(ck, raw))) == oracle.msm(0, bases, raw, threads=8)
    c = Circuit.for_resolution("contrast", "HD")
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-secondary")
    ivc = hip.IVC(ctx, c, ck, ck2, max_batch=4)
    try:
        z0, inputs = step_inputs("contrast")
        ivc.reset(z0); ivc.fold(np.stack(inputs[:8]))
        E = np.ascontiguousarray(ivc.export(0, hip.IX_RUNNING_E))
        inst = from_limbs(ivc.export(0, hip.IX_INSTANCE))
    finally:
        ivc.close(); ck2.free()
    assert (E == 0).all(axis=1).mean() > 0.2                    # it IS the structured vector, not a dense one
    want = oracle.msm(0, bases[:len(E)], E, threads=8)
    assert want == (inst[2], inst[3])                           # the prover's comm_E is the oracle's commitment to E
    pad = np.zeros((n, 4), dtype=np.uint64); pad[:len(E)] = E
    assert tuple(from_limbs(ctx.msm(ck, pad))) == want
    v = ctx.vec_from_host(_lib.FIELD_BN254_FR, E)
    assert tuple(from_limbs(ctx.msm_vec(ck, v))) == want
    v.free(); ck.free()


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_commitment_key_derivation(ctx, oracle, cid):
    """GPU SHAKE256 try-and-increment generators == Python hashlib restatement; all on the curve."""
    from tests._oracle import ck_derive
    n = 300
    B = ctx.bases_generate(cid, n, label=b"ck")
    pts = B.download()
    B.free()
    for i in list(range(40)) + [n - 1]:
        got = tuple(from_limbs(pts[i]))
        assert got == ck_derive(cid, b"ck", i), i
        assert oracle.on_curve(cid, got)
    B2 = ctx.bases_generate(cid, 8, label=b"other")
    assert tuple(from_limbs(B2.download()[0])) == ck_derive(cid, b"other", 0) != tuple(from_limbs(pts[0]))
    B2.free()


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_msm_with_window_tables(ctx, oracle, cid):
    """Precomputed window tables (one shared bucket set, no Horner) give the same points as the oracle: dense scalars,
    witness-like scalars with the unit split, sub-ranges with a base offset, and an explicit window override (classic path)."""
    from vimz_amd import _lib
    r = MODULI[CURVE_SCALAR[cid]]
    n = 6000
    rng = random.Random(31 + cid)
    bases = oracle.seq_bases(cid, n)
    bases[11] = 0                                              # an identity base stays the identity in every table row
    dense = [rng.randrange(r) for _ in range(n)]
    dense[:6] = [0, 1, r - 1, 1 << 200, 65535, 65536]
    wit = [rng.choice([0, 1, 1, rng.randrange(256), rng.randrange(r)]) for _ in range(n)]
    B = ctx.bases_upload(cid, bases).precompute()
    try:
        for sc, split in ((dense, False), (wit, True), (wit, False)):
            v = ctx.vec_from_host(CURVE_SCALAR[cid], to_limbs(sc))
            assert tuple(from_limbs(ctx.msm_vec(B, v, split_ones=split))) == oracle.msm(cid, bases, to_limbs(sc), threads=8)
            assert tuple(from_limbs(ctx.msm_vec(B, v, n=700, offset=100, base_offset=300, split_ones=split))) == \
                oracle.msm(cid, bases[300:1000], to_limbs(sc[100:800]), threads=8)
            assert tuple(from_limbs(ctx.msm_vec(B, v, window_bits=9))) == oracle.msm(cid, bases, to_limbs(sc), threads=8)
            v.free()
        if cid == 0:
            B.precompute(12)                                   # another table width
            v = ctx.vec_from_host(CURVE_SCALAR[cid], to_limbs(dense))
            assert tuple(from_limbs(ctx.msm_vec(B, v))) == oracle.msm(cid, bases, to_limbs(dense), threads=8)
            v.free()
    finally:
        B.free()


@pytest.mark.gpu
def test_msm_with_per_window_tables(ctx, oracle):
    """Tables of the large-MSM window (11 bits) keep the per-window bucket sets and only spare the host its Horner: same points as the
    oracle on dense and witness-like scalars (unit split), on a sub-range with a base offset, and on an MSM too small for that window
    (which ignores the tables)."""
    cid = 0
    r = MODULI[CURVE_SCALAR[cid]]
    n = 1 << 15
    rng = random.Random(77)
    bases = oracle.seq_bases(cid, n)
    bases[5] = 0
    dense = [rng.randrange(r) for _ in range(n)]
    dense[:6] = [0, 1, r - 1, 1 << 200, 65535, 65536]
    wit = [rng.choice([0, 1, 1, rng.randrange(256), rng.randrange(r)]) for _ in range(n)]
    B = ctx.bases_upload(cid, bases).precompute(11)
    try:
        for sc, split in ((dense, False), (wit, True)):
            v = ctx.vec_from_host(CURVE_SCALAR[cid], to_limbs(sc))
            assert tuple(from_limbs(ctx.msm_vec(B, v, split_ones=split))) == oracle.msm(cid, bases, to_limbs(sc), threads=8)
            assert tuple(from_limbs(ctx.msm_vec(B, v, n=n - 64, offset=32, base_offset=17, split_ones=split))) == \
                oracle.msm(cid, bases[17:17 + n - 64], to_limbs(sc[32:n - 32]), threads=8)
            assert tuple(from_limbs(ctx.msm_vec(B, v, n=30000, split_ones=split))) == oracle.msm(cid, bases[:30000], to_limbs(sc[:30000]), threads=8)
            v.free()
    finally:
        B.free()



@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_msm_over_tables_of_multiples(ctx, oracle, cid):
    """vimz_bases_precompute(7): every multiple m·2^(7w)·P_i resident, the MSM is one sum of selected points (k_msm_fixed — what the
    per-step commitments over the verifier circuits' key slices use).  Same points as the oracle on every curve: dense scalars with the
    edge values (0, 1, r−1: the all-ones digits and the top-window carry of a 254 / 255-bit modulus, ±64 digits), witness-like scalars,
    all-equal scalars (every lane of a tree the same point: the doubling branch of the four-lane addition), an identity base,
    sub-ranges with offsets, one workgroup per window and several."""
    r = MODULI[CURVE_SCALAR[cid]]
    rng = random.Random(91 + cid)
    for n in (5000, 700, 1025):
        bases = oracle.seq_bases(cid, n)
        bases[7] = 0
        dense = [rng.randrange(r) for _ in range(n)]
        dense[:10] = [0, 1, r - 1, 1 << 200, 64, 65, 63, 128 - 64, (1 << 254) % r, r - 64]
        wit = [rng.choice([0, 1, 1, rng.randrange(256), rng.randrange(r)]) for _ in range(n)]
        same = [dense[20]] * n
        B = ctx.bases_upload(cid, bases).precompute(7)
        try:
            for sc in (dense, wit, same):
                v = ctx.vec_from_host(CURVE_SCALAR[cid], to_limbs(sc))
                assert tuple(from_limbs(ctx.msm_vec(B, v))) == oracle.msm(cid, bases, to_limbs(sc), threads=8)
                if n > 1000:
                    assert tuple(from_limbs(ctx.msm_vec(B, v, n=600, offset=100, base_offset=300))) == oracle.msm(cid, bases[300:900], to_limbs(sc[100:700]), threads=8)
                    assert tuple(from_limbs(ctx.msm_vec(B, v, n=1, offset=3, base_offset=9))) == oracle.msm(cid, bases[9:10], to_limbs(sc[3:4]), threads=8)
                v.free()
        finally:
            B.free()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [2, 3, 1])
def test_msm_general_pipeline_on_the_255_bit_curves_at_2_17(ctx, oracle, cid):
    """n = 2^17 through the GENERAL pipeline (k_hist_lds -> k_accum -> k_combine -> k_reduce; VERDICT r2: Pasta parity stopped at 6 000
    points) on Pallas and Vesta — whose 255-bit scalars reach the top window's carry path that 254-bit BN scalars never do — and on
    Grumpkin: dense full-width scalars, all-(q−1) (every digit −1 with a carry into the last window: one bucket per window holds every
    point), witness-like scalars with the unit split, and a sub-range with offsets; plus linearity at full size."""
    q = MODULI[CURVE_SCALAR[cid]]
    n = 1 << 17
    rng = random.Random(170 + cid)
    bases = oracle.seq_bases(cid, n)
    bases[12345] = 0
    B = ctx.bases_upload(cid, bases)
    try:
        dense = [rng.randrange(q) for _ in range(n)]
        dense[:8] = [0, 1, q - 1, q - 2, (q - 1) // 2, 1 << 254 if (1 << 254) < q else (1 << 253), (1 << 11) - 1, 1 << 11]
        d_l = to_limbs(dense)
        want = oracle.msm(cid, bases, d_l, threads=8)
        assert tuple(from_limbs(ctx.msm(B, d_l))) == want
        allm1 = to_limbs([q - 1] * n)
        assert tuple(from_limbs(ctx.msm(B, allm1))) == oracle.msm(cid, bases, allm1, threads=8)
        wit = to_limbs([rng.choice([0, 1, 1, 1, rng.randrange(256), rng.randrange(q)]) for _ in range(n)])
        v = ctx.vec_from_host(CURVE_SCALAR[cid], wit)
        w_want = oracle.msm(cid, bases, wit, threads=8)
        assert tuple(from_limbs(ctx.msm_vec(B, v, split_ones=True))) == w_want
        assert tuple(from_limbs(ctx.msm_vec(B, v))) == w_want
        assert tuple(from_limbs(ctx.msm_vec(B, v, n=100000, offset=777, base_offset=4321))) == oracle.msm(cid, bases[4321:104321], wit[777:100777], threads=8)
        v.free()
        # linearity at full size: MSM(s) + MSM(q − s) = identity·(...) : s + (q − s) ≡ 0
        neg = to_limbs([(q - s) % q for s in dense])
        assert oracle.curve_add(cid, want, tuple(from_limbs(ctx.msm(B, neg)))) == (0, 0)
    finally:
        B.free()


@pytest.mark.gpu
def test_kzg_style_commitment_over_an_uploaded_srs_has_the_closed_form_value(ctx, oracle):
    """The Sonobe backend commits with KZG over BN254 G1 (vimz/src/sonobe_backend/folding.rs:22: `KZG<'static, Bn254>`): an MSM over
    the SRS's powers [tau^i]G, handed to this library as an ordinary key (`vimz_bases_upload`).  With a test SRS whose tau is known the
    commitment has a closed form that needs no other MSM to check it:  sum_i c_i·[tau^i]G = p(tau)·G.  Dense coefficients, 2^14
    powers, and a sub-range (a polynomial of lower degree times a power of tau)."""
    r = MODULI[0]
    n = 1 << 14
    tau = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % r
    G = GENERATORS[0]
    powers, t = [], 1
    for _ in range(n):
        powers.append(t)
        t = t * tau % r
    srs = np.zeros((n, 8), dtype=np.uint64)
    for i, k in enumerate(powers):
        srs[i] = to_limbs(list(oracle.curve_mul(0, G, k))).reshape(-1)
    B = ctx.bases_upload(0, srs)
    try:
        rng = random.Random(2718)
        coeffs = [rng.randrange(r) for _ in range(n)]
        p_tau = sum(c * k for c, k in zip(coeffs, powers)) % r
        assert tuple(from_limbs(ctx.msm(B, to_limbs(coeffs)))) == oracle.curve_mul(0, G, p_tau)
        v = ctx.vec_from_host(0, to_limbs(coeffs))
        q_tau = sum(c * k for c, k in zip(coeffs[100:5100], powers[300:5300])) % r
        assert tuple(from_limbs(ctx.msm_vec(B, v, n=5000, offset=100, base_offset=300))) == oracle.curve_mul(0, G, q_tau)
        # KZG openings (vimz_kzg_open: what Sonobe's decider produces for the final commitments, decider.rs:13-21): eval = p(z) and
        # proof = commit((p(X) - p(z)) / (X - z)); with tau known the proof has the closed form ((p(tau) - p(z)) / (tau - z))·G, and the
        # pairing equation e(proof, [tau - z]H) = e(comm - eval·G, H) becomes (tau - z)·proof == comm - eval·G in G1
        for z in (5, rng.randrange(r), tau + 1, 0):
            ev, proof = ctx.kzg_open(B, v, z)
            p_z = sum(c * pow(z, i, r) for i, c in enumerate(coeffs)) % r
            assert ev == p_z
            want = (p_tau - p_z) * pow((tau - z) % r, -1, r) % r
            assert proof == oracle.curve_mul(0, G, want)
            comm = oracle.curve_mul(0, G, p_tau)
            lhs = oracle.curve_mul(0, proof, (tau - z) % r)
            rhs = oracle.curve_add(0, comm, oracle.curve_mul(0, G, (r - p_z) % r))
            assert lhs == rhs
        # a sub-range of the vector over the low powers, and a constant
        ev, proof = ctx.kzg_open(B, v, 7, n=3000, offset=200)
        sub = coeffs[200:3200]
        p7, pt = sum(c * pow(7, i, r) for i, c in enumerate(sub)) % r, sum(c * k for c, k in zip(sub, powers)) % r
        assert ev == p7 and proof == oracle.curve_mul(0, G, (pt - p7) * pow((tau - 7) % r, -1, r) % r)
        ev, proof = ctx.kzg_open(B, v, 9, n=1, offset=3)
        assert ev == coeffs[3] and proof == (0, 0)
        v.free()
    finally:
        B.free()
