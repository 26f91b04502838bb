"""The integer reference of the MSM head's stage tests (tests/_msm_head_ref.py) checked on the CPU: its digit models against tests/_signed_scalars.digits and against
the scalars they recode; its sort, accumulate, window-sum and unit-sum references folded to whole MSMs against the oracle's; and the case tables hold every edge the
GPU test (tests/test_gpu_msm_head.py) is there for — named one by one, with the coverage conditions (every sub-bucket length, every agg_atomic_inc pattern, every
chunk count) asserted on the tables themselves, so that a later edit cannot drop one silently."""
import random

import numpy as np
import pytest

from tests import _msm_head_ref as H
from tests import _msm_tail_ref as T
from tests._signed_scalars import boundary_values, digits


@pytest.fixture(scope="module")
def orc():
    from tests import _oracle
    return _oracle.load()


ALL_C = sorted({c for c, _ in H.SORT_C_LDS + H.SORT_C_GLOBAL})


@pytest.mark.parametrize("field", H.FIELDS)
def test_the_digit_models_agree_with_the_signed_scalars_model_and_recode_the_scalar(field):
    p = H.FIELD_P[field]
    rng = random.Random(f"head-host/{field}")
    for c in ALL_C:
        K = H.windows(p, c)
        half = 1 << (c - 1)
        for s in H.edge_scalars(p, c) + [rng.randrange(p) for _ in range(40)]:
            d = H.signed_digits(s, c, K)
            assert d == digits(s, c, p) and len(d) == K
            assert sum(x << (c * w) for w, x in enumerate(d)) == s and all(-half < x <= half for x in d)
    K = H.windows(p, 7)
    for s in H.edge_scalars(p, 7) + [rng.randrange(p) for _ in range(200)]:
        assert [H.signed_digit7(s, w) for w in range(K)] == digits(s, 7, p)
    # a digit of exactly half stays positive; half + 1 goes negative with a carry — in the bottom window and in an upper one
    assert H.signed_digits(64, 7, 3) == [64, 0, 0] and H.signed_digits(65, 7, 3) == [-63, 1, 0] and H.signed_digits(65 << 7, 7, 3) == [0, -63, 1]
    assert H.signed_digit7(64, 0) == 64 and H.signed_digit7(65, 0) == -63 and H.signed_digit7(65, 1) == 1
    # 2^k - 1: a carry through every window below k; p - 1 without sgn: a carry into the top window
    d = H.signed_digits((1 << 70) - 1, 7, 12)
    assert d == [-1] + [0] * 9 + [1, 0]
    top = H.signed_digits(p - 1, 16, H.windows(p, 16))
    assert top[-1] > 0 and sum(x << (16 * w) for w, x in enumerate(top)) == p - 1


@pytest.mark.parametrize("field", H.FIELDS)
def test_the_loader_model_skips_flips_and_converts(field):
    p = H.FIELD_P[field]
    r1 = H.R256 % p
    for form in H.FORMS:
        unit = H.to_form(1, p, form)
        assert unit == (r1 if form else 1)
        assert H.load_scalar(0, p, form, 0, 1) is None
        assert H.load_scalar(unit, p, form, 1, 1) is None and H.load_scalar(unit, p, form, 0, 1) == (1, 0)
        for w in H.near_units(p, form):          # share all 32-bit words but one with the unit, and are not skipped
            assert w != unit and sum(1 for k in range(8) if (w >> (32 * k)) & 0xffffffff != (unit >> (32 * k)) & 0xffffffff) == 1
            assert H.load_scalar(w, p, form, 1, 0) is not None
        assert len(H.near_units(p, form)) >= 7
        lo, hi = (p - 1) // 2, (p + 1) // 2
        assert H.load_scalar(H.to_form(lo, p, form), p, form, 0, 1) == (lo, 0)
        assert H.load_scalar(H.to_form(hi, p, form), p, form, 0, 1) == (p - hi, 1) == (lo, 1)
        assert H.load_scalar(H.to_form(hi, p, form), p, form, 0, 0) == (hi, 0)
        assert H.load_scalar(H.to_form(p - 1, p, form), p, form, 1, 1) == (1, 1)      # -1 is not the unit
        for s in boundary_values(p):
            ls = H.load_scalar(H.to_form(s, p, form), p, form, 0, 1)
            assert ls is None if s == 0 else (ls[0] if not ls[1] else p - ls[0]) == s and 2 * ls[0] <= p - 1 + (1 - ls[1])


def _live(ks, words):
    """the pairs an oracle MSM is given: the identity bases dropped (they add nothing)"""
    return [(k, w) for k, w in zip(ks, words) if k]


def _oracle_msm(orc, c, ks, canon):
    from tests._oracle import to_limbs
    pairs = _live(ks, canon)
    if not pairs:
        return (0, 0)
    return tuple(orc.msm(c, H.key_points(c, [k for k, _ in pairs]), to_limbs([s for _, s in pairs]), threads=2))


@pytest.mark.parametrize("c", H.CURVES)
def test_the_references_fold_to_the_oracles_msm(c, orc):
    f = H.SCALAR_FIELD[c]
    p = H.FIELD_P[f]
    ri = pow(H.R256, -1, p)
    n = 150
    ks = H.key_ks(n)
    assert 0 in ks and any(k < 0 for k in ks) and len(set(ks)) < len(ks)
    pts = H.key_points(c, ks[:12])
    assert all(T.on_curve(c, _xy(r)) for r in pts) and _xy(pts[3]) == (0, 0)
    for form in H.FORMS:
        words = H.scalar_words(f, n, 7, form)
        canon = [w * ri % p if form else w for w in words]
        want = _oracle_msm(orc, c, ks, canon)
        assert want == T.mul(c, H.msm_scalar(c, words, ks, form))
        for sgn in (0, 1):
            # the fused paths' window sums: Horner without tables, added with them
            for tables in (0, 1):
                sums = H.window_sums_ref(c, words, ks, form, sgn, tables)
                assert T.mul(c, H.fold_window_sums(c, sums, tables)) == want, (form, sgn, tables)
            # the sort's entries: bucket sums, weighted, then Horner over the windows (per-window sets) — and with a table row stride the entry still names its point
            for cb, shared in ((5, 0), (12, 0), (16, 1)):
                K = H.windows(p, cb)
                nbw = 1 << (cb - 1)
                nb, bstride, pstride = (nbw, 0, n + 3) if shared else (nbw * K, nbw, 0)
                counts, boff, soff, totals, ent = H.sort_ref(words, p, form, 0, sgn, cb, K, bstride, pstride, nb, 8)
                assert totals[1] == len(ent) == int(counts.sum()) and totals[0] == int(((counts + 7) // 8).sum()) and boff[-1] == len(ent)
                acc = 0
                for g, v in ent:
                    idx, neg = v & 0x7fffffff, v >> 31
                    w, i = (idx // pstride, idx % pstride) if shared else (g // nbw, idx)
                    assert i < n and w < K
                    acc += (-1 if neg else 1) * (g % nbw + 1) * ks[i] << (cb * w)
                assert T.mul(c, acc) == want, (form, sgn, cb)
        # the unit sums
        ow = H.ones_words(c, n, form, "mixed")
        one = H.to_form(1, p, form)
        assert 10 < ow.count(one) < n
        assert T.mul(c, H.ones_ref(ow, ks, p, form)) == _oracle_msm(orc, c, ks, [1 if w == one else 0 for w in ow])
    # the accumulate reference: the partials of a row add up to the sum of its entries
    for sub in H.ACCUM_SUB:
        srt, boff, soff, totals, layouts = H.accum_arrays(sub, 257, 3)
        for r, lay in enumerate(layouts):
            ref = H.accum_ref(lay, sub)
            assert len(ref) == 257 == totals[r, 0]
            flat = [e for b in lay for e in b]
            acc = (0, 0)
            for i, s in flat:
                pt = T.mul(c, H.ACCUM_KEY[i])
                acc = orc.curve_add(c, acc, T.neg(c, pt) if s else pt)
            assert tuple(acc) == T.mul(c, sum(ref))


def _xy(row):
    return tuple(int(row[4 * k]) | int(row[4 * k + 1]) << 64 | int(row[4 * k + 2]) << 128 | int(row[4 * k + 3]) << 192 for k in (0, 1))


def test_the_sub_bucket_length_model_and_its_distributions():
    assert H.small_sub_len([0] * 64) == 4 and H.small_sub_len([16] * 64) == 4 and H.small_sub_len([1536] + [0] * 63) == 6 and H.small_sub_len([24] * 64) == 6
    for want, counts in H.SUBLEN_DISTRIBUTIONS.items():
        assert len(counts) == 64 and sum(counts) <= H.SMALL_CHUNK and H.small_sub_len(counts) == want
        assert sum((n + want - 1) // want for n in counts) <= H.SMALL_THREADS
        if want > 4:
            assert sum((n + want - 2) // (want - 1) for n in counts) > H.SMALL_THREADS
    # every length is reached by some (case, window, chunk) of the table — the crafted chunks in window 0, as built
    cases = H.small_cases()
    reached = {}
    for name, case in cases.items():
        if case["curve"] == 1 and (name.startswith("crafted/") or case["n"] in (1536, 1537)):
            for (w, q), sub in H.chunk_sublens(case).items():
                reached.setdefault(sub, (name, w, q))
    assert set(reached) == {4, 5, 6, 7, 8}, reached
    for want in (4, 5, 6, 7, 8):
        case = cases[f"crafted/{H.CURVE_NAMES[1]}/sublen_{want}"]
        assert H.chunk_sublens(case)[(0, 0)] == want
    # one bucket of 1536 entries: 256 sub-buckets of 6 (the shortest that fits), a segmented tree of depth 8
    sc, ks = H.crafted("one_value_1536")
    cnt = H.chunk_bucket_counts([H.signed_digit7(s, 0) for s in sc])
    assert cnt[4] == 1536 and sum(cnt) == 1536 and H.small_sub_len(cnt) == 6 and (1536 // 6 - 1).bit_length() == 8
    sc, ks = H.crafted("one_per_bucket")
    assert H.chunk_bucket_counts([H.signed_digit7(s, 0) for s in sc]) == [1] * 64
    sc, ks = H.crafted("bucket_63_alone")
    assert [H.signed_digit7(s, 0) for s in sc] == [64]
    sc, ks = H.crafted("identity_under_negative_digit")
    assert all(H.signed_digit7(s, 0) < 0 for s in sc) and ks.count(0) == 20
    sc, ks = H.crafted("all_bases_equal")
    assert len(set(ks)) == 1 and {d > 0 for d in (H.signed_digit7(s, 0) for s in sc)} == {True, False}
    sc, ks = H.crafted("p_next_to_minus_p")
    d = [H.signed_digit7(s, 0) for s in sc]
    assert (d[0], ks[0]) == (d[1], -ks[1]) and (d[2], ks[2]) == (-d[3], ks[3]) and d[4:] == [64] * 3 and sum(dd * k for dd, k in zip(d, ks)) == 64 * 11


def test_the_agg_cases_hold_every_pattern_of_agg_atomic_inc():
    cases = H.sort_cases()
    pats = {}
    for name, case in cases.items():
        if not name.startswith("agg/"):
            continue
        assert case["lds"] == 0 and case["n"] == H.AGG_N and H.AGG_N % 64 != 0
        words = H.sort_words(case)
        p = H.FIELD_P[case["field"]]
        ri = pow(H.R256, -1, p)
        distinct, zeros = case["kind"][1], case["kind"][2]
        for run in range(4):
            lanes = [w * ri % p if case["form"] else w for w in words[64 * run:64 * run + 64]]
            live = [x for x in lanes if x]
            assert len(set(live)) == min(distinct, len(live)) and (len(live) == 64) == (not zeros)
            assert all(0 < x <= 1 << (case["c"] - 1) for x in live)          # one digit each, in window 0: one counter a lane
            pats.setdefault(H.agg_pattern(lanes), name)
    assert {d for n, c in cases.items() if n.startswith("agg/") for d in [c["kind"][1]]} == set(H.AGG_DISTINCT) == {1, 2, 3, 5, 16, 64}
    assert {c["c"] for n, c in cases.items() if n.startswith("agg/")} == {7, 12, 16}
    rounds = {r for r, _, _ in pats}
    assert rounds == {1, 2, 3, 4}, pats                                               # one to four leader rounds
    assert any(fb == 0 and not early for _, fb, early in pats)                        # everybody served by a leader
    assert any(early and fb > 0 for _, fb, early in pats)                             # the early break, the rest per lane
    assert any(r == 4 and fb > 0 and not early for r, fb, early in pats)              # four full rounds, then the per-lane fallback
    assert any(r == 1 and early and fb >= 42 for r, fb, early in pats)                # every lane its own counter


def test_the_case_tables_hold_every_named_edge():
    # sort
    assert H.SORT_C_LDS == ((2, 0), (5, 0), (7, 0), (11, 0), (15, 1), (16, 1)) and H.SORT_C_GLOBAL == ((7, 0), (12, 0), (16, 1))
    assert H.SORT_N == (1, 63, 64, 65, 1023, 1024, 1025, 4097) and H.SORT_BLOCKS == (1, 2, 32, 256)
    sc = H.sort_cases()
    grid = {n: c for n, c in sc.items() if n.startswith("grid/")}
    assert len(grid) == 9 * 8 and {(c["lds"], c["c"], c["shared"], c["n"]) for c in grid.values()} == \
        {(lds, cb, sh, n) for lds, tab in ((1, H.SORT_C_LDS), (0, H.SORT_C_GLOBAL)) for cb, sh in tab for n in H.SORT_N}
    for key, vals in (("field", H.FIELDS), ("form", H.FORMS), ("sgn", (0, 1)), ("skip_ones", (0, 1)), ("sub", H.SORT_SUB)):
        assert {c[key] for c in grid.values()} == set(vals)
    assert {c["sort_blocks"] for c in grid.values() if c["lds"]} == set(H.SORT_BLOCKS)
    combos = {(c["field"], c["form"], c["sgn"], c["skip_ones"], c["lds"]) for n, c in sc.items() if n.startswith("combo/")}
    assert len(combos) == 4 * 2 * 2 * 2 * 2
    assert any(c["lds"] and c["n"] < c["sort_blocks"] for c in sc.values())                                        # workgroups with an empty chunk
    assert any(c["lds"] and c["n"] > c["sort_blocks"] > 1 and c["n"] % -(-c["n"] // c["sort_blocks"]) for c in sc.values())      # a short last chunk
    for c in sc.values():
        K, nbw, nb, bstride, pstride = H.sort_shape(c)
        assert not c["lds"] or nb * 4 <= H.LDS_LIMIT
        assert (pstride > c["n"]) == bool(c["shared"])
    assert any(H.sort_shape(c)[2] * 4 > H.LDS_LIMIT for c in sc.values() if not c["lds"])                          # the fallback where the LDS sort does not fit
    for field in H.FIELDS:
        p = H.FIELD_P[field]
        for form in H.FORMS:
            words = H.scalar_words(field, 1025, 11, form)
            canon = {w * pow(H.R256, -1, p) % p if form else w for w in words}
            assert set(boundary_values(p)) <= canon and {(p - 1) // 2, (p + 1) // 2, 1 << 10, (1 << 10) + 1, p - 1, 0, 1} <= canon
            assert {(1 << k) - 1 for k in range(1, p.bit_length())} <= canon
            assert set(H.near_units(p, form)) & set(words)
            assert H.scalar_words(field, 1, 11, form) == [H.to_form(p - 1, p, form)]
    zero = sc["all_zero/field=0/form=0/lds=1"]
    assert H.sort_ref(H.sort_words(zero), H.FIELD_P[0], 0, 0, 1, 7, 37, 64, 0, 64 * 37, 8)[3] == [0, 0, 0, 0]
    for skip, entries in ((0, 65), (1, 0)):
        one = sc[f"all_one/field=1/form=1/skip_ones={skip}/lds=0"]
        assert H.sort_ref(H.sort_words(one), H.FIELD_P[1], 1, skip, 1, 7, 37, 64, 0, 64 * 37, 8)[3][1] == entries
    # accumulate
    assert H.ACCUM_SUB == (8, 16) and H.ACCUM_TOTALS == (0, 1, 255, 256, 257) and H.ACCUM_ROWS == (1, 3, 16)
    assert {(s, t) for s, t, _ in H.ACCUM_CASES} == {(s, t) for s in H.ACCUM_SUB for t in H.ACCUM_TOTALS} and {r for _, _, r in H.ACCUM_CASES} == set(H.ACCUM_ROWS)
    assert H.ACCUM_KEY[0] == 0 and H.ACCUM_KEY[41] == H.ACCUM_KEY[5] and H.ACCUM_KEY[42] == -H.ACCUM_KEY[6]
    assert set(H.ACCUM_PLANTED) == {"doubling_first", "doubling_mid_chain", "same_point_other_index", "cancel_then_more", "cancel_mid_chain", "negated_base_cancels",
                                    "identity_first", "identity_first_signed", "identity_middle", "identity_middle_signed", "identity_last", "identity_last_signed",
                                    "identity_alone_signed"}
    k = lambda piece, upto: sum(-H.ACCUM_KEY[i] if s else H.ACCUM_KEY[i] for i, s in piece[:upto])      # noqa: E731
    pl = H.ACCUM_PLANTED
    assert k(pl["doubling_mid_chain"], 2) == H.ACCUM_KEY[pl["doubling_mid_chain"][2][0]] and k(pl["cancel_mid_chain"], 3) == 0 and k(pl["cancel_then_more"], 2) == 0
    assert k(pl["negated_base_cancels"], 2) == 0 and k(pl["doubling_first"], 1) == H.ACCUM_KEY[pl["doubling_first"][1][0]]
    for sub in H.ACCUM_SUB:
        for total in (255, 256, 257):
            lay = H.accum_layout(sub, total)
            sizes = [len(b) for b in lay]
            assert {sub - 1, sub, sub + 1, 2 * sub} <= set(sizes) and sum((s + sub - 1) // sub for s in sizes) == total
            runs = "".join("e" if s == 0 else "f" for s in sizes)
            assert runs.startswith("eeeee") and runs.endswith("eee") and "f" + "e" * 67 + "f" in runs
            for piece in pl.values():
                assert any(b[-len(piece):] == piece or b[:len(piece)] == piece for b in lay)
            assert any(len(b) == sub + len(pl["doubling_mid_chain"]) and b[sub:] == pl["doubling_mid_chain"] for b in lay)      # a planted piece alone in a bucket's second piece
        assert all(len(b) == 0 for b in H.accum_layout(sub, 0)) and sum(len(b) for b in H.accum_layout(sub, 1)) == 1
    # fused small
    assert H.SMALL_N_Q1 == (1, 255, 256, 257, 1536) and H.SMALL_Q_CHUNK3 == (2, 3, 4, 5, 7, 8, 20)
    sm = H.small_cases()
    for c in H.CURVES:
        mine = [x for x in sm.values() if x["curve"] == c]
        shapes = {(x["n"], x["Q"], x["chunk"]) for x in mine if x["kind"] == "edges"}
        assert {(n, 1, n) for n in H.SMALL_N_Q1} | {(1537, 2, 769)} | {(3 * Q - 1, Q, 3) for Q in H.SMALL_Q_CHUNK3} <= shapes
        assert {x["Q"] for x in mine} >= {1, 2, 3, 4, 5, 7, 8, 20}                                               # every Q listed occurs
        assert {(x["form"], x["sgn"], x["tail"], x["calls"]) for x in mine if x["Q"] == 3 and x["n"] == 8} == {(f, s, t, k) for f in (0, 1) for s in (0, 1) for t in (0, 1) for k in (1, 2)}
        assert {x["kind"] for x in mine} == set(H.CRAFTED) | {"edges"}
        assert any(x["tables"] and x["offset"] > 0 for x in mine) and any(x["tables"] and x["Q"] > 1 for x in mine)
        assert {x["tail"] for x in mine if x["Q"] > 1 and x["kind"] == "edges" and x["n"] != 8} == {0, 1}
    assert (30720, 20, 1536) in {(x["n"], x["Q"], x["chunk"]) for x in sm.values() if x["curve"] == H.SMALL_BIG_CURVE}
    assert all(x["n"] is None or x["chunk"] * (x["Q"] - 1) < x["n"] <= x["chunk"] * x["Q"] for x in sm.values())
    assert {Q % 3 for Q in H.SMALL_Q_CHUNK3} == {0, 1, 2} and min(H.SMALL_Q_CHUNK3) <= 4 < max(H.SMALL_Q_CHUNK3)
    # fixed-base and the tables
    assert H.FIXED_N == (1, 255, 256, 257, 1024, 1025) and H.FIXED_BIG_N == (2049, 4097)
    fx = H.fixed_cases()
    for c in H.CURVES:
        assert {(x["n"], x["calls"]) for x in fx.values() if x["curve"] == c} >= {(n, k) for n in H.FIXED_N for k in (1, 2)}
        assert any(x["offset"] for x in fx.values() if x["curve"] == c)
    assert {-(-x["n"] // H.FIXED_CHUNK) for x in fx.values()} == {1, 2, 3, 5}                                    # Qf: one workgroup, two, a padded tree of three, of five
    assert H.TABLE_C == (7, 11, 15) and H.TABLE_N == (1, 255, 256, 257) and H.TABLE_M == (1, 2, 63, 64) and len(H.table_cases()) == 4 * 3 * 4
    for c, tc, n in H.table_cases():
        ent = H.table_entries(c, tc, n)
        K = H.windows(H.FIELD_P[H.SCALAR_FIELD[c]], tc)
        assert {e[1] for e in ent} == {0, 1, K - 1} and {e[2] for e in ent} == {0, n // 2, n - 1}
        assert (n <= 2) or any(e[4] == 0 for e in ent)                                                             # the identity base
        assert ({e[3] for e in ent if e[0] == 1} == set(H.TABLE_M)) == (tc == 7)
    # unit sums
    assert H.ONES_N == (1, 63, 64, 65, 128, 129) and H.ONES_BIG_N == 3 * 16384 + 64 and H.ONES_ROWS == (1, 2, 32)
    on = H.ones_cases()
    for c in H.CURVES:
        for form in H.FORMS:
            mine = [x for x in on.values() if x["curve"] == c and x["form"] == form]
            assert {(x["n"], x["kind"]) for x in mine} >= {(n, k) for n in H.ONES_N + (H.ONES_BIG_N,) for k in H.ONES_KINDS}
            assert {x["content"] for x in mine} >= {"queue", "no_units", "near_units", "mixed", "all_units"}
        assert {x["rows"] for x in on.values() if x["curve"] == c and x["kind"] == 2} == set(H.ONES_ROWS)
    for form in H.FORMS:
        p = H.FIELD_P[H.SCALAR_FIELD[0]]
        words = H.ones_words(0, H.ONES_BIG_N, form, "queue")
        fills = [H.queue_fills(words, p, form, w) for w in range(4)]
        assert fills[0][:3] == [63, 64, 0] and fills[1][:3] == [63, 127, 63] and fills[2][:3] == [64, 0, 1] and fills[3][:3] == [0, 0, 1]
        assert len(fills[0]) == 4 and fills[0][3] == 2 and len(fills[1]) == 3                                      # wave 0's short fourth pass
        assert H.ones_ref(H.ones_words(0, 129, form, "no_units"), H.key_ks(129), p, form) == 0
        one = H.to_form(1, p, form)
        assert one not in H.ones_words(0, 65, form, "near_units") and one not in H.ones_words(0, 129, form, "no_units")
    # invalid layouts and the groups
    assert len(H.INVALID) == 16 and len(set(H.INVALID)) == 16
    assert H.GROUPS == ("sort", "accum", "small", "fixed", "tables", "ones", "invalid") and all(H.group_cases(g) for g in H.GROUPS)
