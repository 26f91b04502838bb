"""The integer reference of the MSM tail's stage tests (tests/_msm_tail_ref.py) checked on the CPU: slots round-trip and the bounds checker refuses what lies
just over each bound; sums by plain additions, by the discrete-log route and by the oracle agree; the reduce references agree with the naive weighted sum; and the
case tables hold every edge the GPU test (tests/test_gpu_msm_tail.py) is there for — named one by one, so that a later edit cannot drop one silently."""
import random

import numpy as np
import pytest

from tests import _msm_tail_ref as T
from tests._fp29_ref import R


@pytest.fixture(scope="module")
def orc():
    from tests import _oracle
    return _oracle.load()


@pytest.mark.parametrize("c", T.CURVES)
def test_slots_round_trip_in_every_representation(c):
    assert T.on_curve(c, T.GENERATOR[c]) and T.mul(c, T.ORDER[c]) == (0, 0) and T.mul(c, T.ORDER[c] - 1) == T.neg(c, T.GENERATOR[c])
    for kind in T.CONTENTS:
        specs = T.content(c, kind, 24, "host")
        slots = T.pack(c, specs)
        assert slots.shape == (24, T.SLOT_WORDS) and slots.dtype == np.uint32
        for spec, slot in zip(specs, slots):
            assert T.unpack(c, slot) == T.mul(c, spec[0])
            assert T.slot_is_identity(slot) == (spec[0] == 0)
    lifted = T.content(c, "max_lifts", 24, "host")
    assert all(s[2] == T.MAX_LIFT for s in lifted)
    reps = T.content(c, "same_point_representations", 24, "host")
    assert len({s[0] for s in reps}) == 1 and len({s[1:] for s in reps}) > 1
    assert not np.array_equal(*T.pack(c, reps[:2])) or reps[0] == reps[1]


def _slot_of_values(vals):
    from tests._fp29_ref import ints_to_limbs29
    out = np.zeros((4, T.COORD_WORDS), dtype=np.uint32)
    out[:, :9] = ints_to_limbs29(list(vals))
    return out.reshape(T.SLOT_WORDS)


@pytest.mark.parametrize("c", T.CURVES)
def test_the_bounds_checker_refuses_a_slot_just_over_each_bound(c):
    p, rng = T.BASE_P[c], random.Random(f"bounds/{c}")
    x, y = T.mul(c, 5)
    for coord, (lift_over, frac) in enumerate(((5, 3), (3, 4), (1, 5), (1, 5))):       # residue >= frac/10 p and lift_over p on top: >= 5.3, 3.4, 1.5, 1.5 p
        while True:
            z = rng.randrange(2, p)
            res = [x * z * z * R % p, y * z ** 3 * R % p, z * z * R % p, z ** 3 * R % p]
            if 10 * res[coord] >= frac * p and all(2 * r < p for r in res[2:] if coord < 2):
                break
        assert T.unpack(c, _slot_of_values(res)) == (x, y)
        under = list(res); under[coord] += (lift_over - 1) * p
        if 10 * under[coord] < T.BOUND_TENTHS[coord] * p:
            assert T.unpack(c, _slot_of_values(under)) == (x, y)
        over = list(res); over[coord] += lift_over * p
        with pytest.raises(T.BadSlot, match="outside its bound"):
            T.unpack(c, _slot_of_values(over))
    good = T.pack(c, [(5, 3, T.NO_LIFT)])[0]
    bad = good.copy(); bad[4] |= 1 << 29
    with pytest.raises(T.BadSlot, match="limb"):
        T.unpack(c, bad)
    bad = good.copy(); bad[30] ^= 1          # ZZZ no longer fits ZZ
    with pytest.raises(T.BadSlot):
        T.unpack(c, bad)
    with pytest.raises(T.BadSlot):
        T.unpack(c, T.garbage(1)[0])
    lying = _slot_of_values([x * R % p, y * R % p, p, p])          # ZZ a non-zero multiple of p is not the identity
    with pytest.raises(T.BadSlot):
        T.unpack(c, lying)


@pytest.mark.parametrize("c", T.CURVES)
def test_sums_by_additions_by_discrete_log_and_by_the_oracle_agree(c, orc):
    from tests._oracle import from_limbs, to_limbs
    for kind in T.CONTENTS:
        ks = [s[0] for s in T.content(c, kind, 40, "sums")]
        plain = T.sum_plain(c, ks)
        assert plain == T.mul(c, sum(ks)), kind
        acc = (0, 0)
        for k in ks:
            acc = orc.curve_add(c, acc, T.mul(c, k))
        assert tuple(acc) == plain, kind
    big = random.Random(f"big/{c}").randrange(T.ORDER[c])
    assert tuple(orc.curve_mul(c, T.GENERATOR[c], big)) == T.mul(c, big)
    assert tuple(orc.curve_mul(c, T.GENERATOR[c], T.POOL + 1)) == T.add(c, T.pool(c)[T.POOL], T.GENERATOR[c]) == T.mul(c, T.POOL + 1)
    bases = orc.seq_bases(c, 64)
    assert [tuple(from_limbs(b)) for b in bases[:3]] == [T.pool(c)[1], T.pool(c)[2], T.pool(c)[3]]
    scalars = [random.Random(f"msm/{c}/{i}").randrange(1 << 40) for i in range(64)]
    assert tuple(orc.msm(c, bases, to_limbs(scalars), threads=2)) == T.mul(c, sum((i + 1) * s for i, s in enumerate(scalars)))


def test_the_reduce_references_equal_the_naive_weighted_sum():
    rng = random.Random("reduce-ref")
    for nbw in (2, 16, 1024):
        ks = [rng.randrange(-50, 50) for _ in range(nbw)]
        counts = [rng.randrange(3) for _ in range(nbw)]
        naive = sum((i + 1) * k for i, (k, n) in enumerate(zip(ks, counts)) if n)
        weighted, plain = T.reduce_ref(ks, counts)
        assert weighted == naive and plain == sum(k for k, n in zip(ks, counts) if n)
        planes = T.planes_ref(ks, counts)
        assert len(planes) == nbw.bit_length() + 1 and T.planes_total(planes) == naive and planes[-2] + planes[-1] == plain
    for c in (0, 2):      # and as points: the window sum of a small window by plain additions
        specs, counts = T.window_specs(c, "zero_counts_over_garbage", 16, "host")
        acc = (0, 0)
        for i, (s, n) in enumerate(zip(specs, counts)):
            for _ in range(i + 1 if n else 0):
                acc = T.add(c, acc, T.mul(c, s[0]))
        assert acc == T.mul(c, T.reduce_ref([s[0] for s in specs], counts)[0])


def test_the_level_model_of_a_tree_sums_into_slot_0():
    c = 0
    for kind in T.CONTENTS:
        specs = T.content(c, kind, 256, "quad", kmax=600)
        ks, limbs = T.apply_levels(specs, T.pack(c, specs), T.TREE256_LEVELS)
        assert ks[0] == T.scalar_sum(specs), kind
        assert all(limbs[i] is not None for i in range(128, 256))          # the upper half is never a destination: limb for limb as it was
    specs, level = T.planted_level(c)
    ks, limbs = T.apply_levels(specs, T.pack(c, specs), [level])
    slots = T.pack(c, specs)
    assert np.array_equal(limbs[0], slots[16]) and ks[0] == specs[16][0] != 0          # copy
    assert np.array_equal(limbs[1], slots[1]) and np.array_equal(limbs[2], slots[2]) and ks[2] == 0      # nothing to store
    assert limbs[3] is None and limbs[4] is None and ks[4] == 2 * specs[4][0] and limbs[5] is None and ks[5] == 30
    assert ks[6] == 0 and not limbs[6].any()                                             # cancellation: the identity
    assert np.array_equal(limbs[7], slots[7]) and np.array_equal(limbs[23], slots[23])   # the inactive quad's would-be operands


def test_the_case_tables_hold_every_named_edge():
    # contents
    assert set(T.CONTENTS) == {"generic", "identity_first_mid_last", "all_identity", "same_point", "same_point_representations", "cancel_pairs",
                               "zero_run_then_more", "max_lifts"}
    ids = [i for i, s in enumerate(T.content(0, "identity_first_mid_last", 17, "x")) if s[0] == 0]
    assert ids == [0, 8, 16]
    zr = [s[0] for s in T.content(0, "zero_run_then_more", 64, "x")]
    assert sum(zr[:32]) == 0 and all(zr) and sum(zr) != 0
    cp = [s[0] for s in T.content(0, "cancel_pairs", 64, "x")]
    assert all(cp[2 * i] == -cp[2 * i + 1] for i in range(32)) and all(cp[e] == -cp[e + 16] for e in range(16))
    # quad levels
    assert T.QUAD_COUNTS == (1, 3, 16, 17, 63, 64) and set(T.QUAD_TABLES) == {"halves", "scattered", "chained"}
    dst, src = T.quad_table("chained", 17)
    assert dst[1:] == src[:-1] and len(set(dst)) == 17
    dst, src = T.quad_table("scattered", 64)
    assert len(set(dst) | set(src)) == 128 and dst != sorted(dst)
    assert T.PLANTED == ("copy_left_identity", "right_identity", "both_identity", "generic", "doubling", "doubling_across_representations", "cancellation",
                         "inactive_quad")
    q = T.group_cases("quad_level")
    assert {x[0] for x in q} == set(T.CURVES) and all((c, "planted", "planted") in q for c in T.CURVES) and len(q) == 4 * 19
    assert len(T.group_cases("quad_tree")) == 4 * 8
    # trees
    assert T.TREE256_M == (1, 2, 255, 256, 257, 16384) and set(T.TREE_ROWS) == {(1, 1), (3, 64), (16, 256), (2, 255)}
    assert len(T.group_cases("tree256")) == 4 * 6 * 8 and len(T.group_cases("tree_rows")) == 16
    # scan
    assert T.SCAN_NB == (1, 1023, 1024, 1025, 7424, 24576) and T.SCAN_SUB == (8, 16) and T.SCAN_BLOCKS == (1, 32, 256)
    assert len(T.group_cases("scan")) == 6 * 6 * 2 * 3 + 1
    for sub in T.SCAN_SUB:
        a = T.scan_counts(1025, "around_multiples_of_sub", sub)
        assert {sub - 1, sub, sub + 1, 2 * sub - 1, 2 * sub, 2 * sub + 1} <= set(a.tolist())
        m = (T.scan_counts(1025, "at_heavy_min", sub).astype(np.int64) + sub - 1) // sub
        assert T.SCAN_HEAVY_MIN in m and T.SCAN_HEAVY_MIN + 1 in m
        assert T.scan_counts(1025, "huge_first", sub)[0] > 1 << 20 and T.scan_counts(1025, "huge_last", sub)[-1] > 1 << 20
    o = T.scan_overflow_counts()
    assert len(o) == 1 << 17 and len(T.scan_ref(o[None, :], 8, T.SCAN_HEAVY_MIN)[3]) == 65537
    h = T.split_over_blocks(T.scan_counts(1023, "at_heavy_min", 8), 32)
    assert h.shape == (32, 1023) and len({tuple(r) for r in h.tolist()}) > 1
    # combine
    for lb in T.COMBINE_LANE_BITS:
        L, hm = 1 << lb, 16 << lb
        want = {0, 1, 2, L, L + 1, 2 * L + 1, hm} | ({L - 1} if L > 1 else set())
        m = T.combine_ordinary_layout(lb)
        per = 256 >> lb
        assert want <= set(m) and max(m) == hm and len(m) % per != 0 and m[per - 1] >= 2 and max(m[per:2 * per]) <= 1 and m[-1] == hm
        assert {f"ordinary/lane_bits={lb}/rows=1", f"ordinary/lane_bits={lb}/rows=3", f"heavy_sizes/lane_bits={lb}"} <= set(T.COMBINE_CASES)
        sizes, ids, n = T.combine_sizes(f"heavy_sizes/lane_bits={lb}")
        assert {hm + 1, 255, 256, 257, 2047} <= set(sizes) and n == len(ids) == len([s for s in sizes if s > hm])
    sizes, ids, n = T.combine_sizes("heavy_513/lane_bits=1")
    assert n == 513 == T.COMBINE_HEAVY_BLOCKS + 1
    sizes, ids, n = T.combine_sizes("split_sizes/calls=2")
    assert {2048, 2049, 4097} <= set(sizes) and T.COMBINE_CASES["split_sizes/calls=2"][2] == 2 and -(-4097 // 32) * 31 < 4097 < -(-4097 // 32) * 32      # a short last part
    sizes, ids, n = T.combine_sizes("split_past_1024/calls=2")
    assert n == 1025 and sizes[ids[1024]] == 2048 and T.COMBINE_CASES["split_past_1024/calls=2"][2] == 2
    sizes, ids, n = T.combine_sizes("split_at_0/calls=2")
    assert n == 1025 and sizes[ids[0]] == 2048 and T.COMBINE_CASES["split_at_0/calls=2"][2] == 2
    sizes, ids, n = T.combine_sizes("overflowed_list")
    assert n == T.HEAVY_CAP + 1 and {17, 300, 2048} <= set(sizes)
    assert T.COMBINE_CASES["split_rows=3/calls=2"][1] == 3
    for name in T.COMBINE_CASES:          # no heavy bucket whose first partial already is its sum: a fold that never ran would pass for one
        for row in range(T.COMBINE_CASES[name][1]):
            sizes = T.combine_sizes(name, row)[0]
            for size, specs in zip(sizes, T.combine_specs(0, name, row)[1]()):
                assert len(specs) == size and (size <= 64 or T.scalar_sum(specs) != specs[0][0]), (name, row, size)
    cc = T.group_cases("combine")
    assert len([x for x in cc if x[0] == 0]) == len(T.COMBINE_CASES) and all(len([x for x in cc if x[0] == c]) == 9 for c in (1, 2, 3))
    # reduce
    assert T.REDUCE_NBW == (2, 16, 128, 256, 512, 1024, 2048) and len(T.REDUCE_BUCKETS) == 8 and set(T.REDUCE_SHAPES) == {(1, 1), (3, 1), (1, 3), (3, 3)}
    for nbw in T.REDUCE_NBW:
        rc = T.reduce_cases(nbw)
        assert {k for _, _, kinds in rc for row in kinds for k in row} == set(T.REDUCE_BUCKETS) and {(W, Rr) for W, Rr, _ in rc} == set(T.REDUCE_SHAPES)
    specs, counts = T.window_specs(0, "only_first_of_last_chunk", 2048, "x")
    assert [i for i, n in enumerate(counts) if n] == [255 * 8]
    specs, counts = T.window_specs(0, "zero_counts_over_garbage", 16, "x")
    assert 0 in counts and 1 in counts
    assert T.REDUCE_MODE1_WINDOWS == (1, 2, 16) and T.REDUCE_PLANES_NBW == (1024, 4096, 16384, 32768) and T.REDUCE_PLANES_G == (1, 4, 16, 8)
    assert len(T.group_cases("reduce")) == 7 * 11 + 3 * 11 and len(T.group_cases("reduce_plain")) == 12 and len(T.group_cases("reduce_planes")) == 4 + 3
    # invalid layouts: one per rule
    assert set(T.INVALID) == {"offsets_not_monotone", "offsets_outside_the_array", "bucket_id_not_below_nb", "index_not_below_256", "dst_twice_in_a_level",
                              "nbw_not_a_power_of_two", "nbw_above_32768", "rows_above_16"}
    assert all(T.group_cases(g) for g in T.GROUPS)
