"""No GPU: the integer reference of the fold step kernels (tests/_fold_ref.py) checked by what it must preserve — the relaxed relation along a chain of folds,
the lookahead identity, the agreement with the seam's cross term and the oracle's — and the generated layouts and case lists checked on the data itself."""
import itertools
import math

import pytest

from tests import _fold_ref as fr
from tests import _seam_cases as sc
from vimz_amd import _lib

FIELDS = [_lib.FIELD_BN254_FR, _lib.FIELD_BN254_FQ, _lib.FIELD_PALLAS_FP, _lib.FIELD_VESTA_FQ]
N, SC, ROWS = fr.SCHEDULE_N, 200, fr.SCHEDULE_ROWS      # the first SC elements are folded by fold_cross, the others by fold5, as a step's rows are


def _chain(fid):
    p = _lib.MODULUS[fid]
    rows = fr.satisfied_rows(p, N, ROWS, f"host:{fid}")
    cls = fr.scalar_classes(p, f"host:{fid}")
    challenges = [cls[3], cls[4], cls[1], cls[3] ^ 5, cls[2], cls[4] ^ 9]      # 128-bit challenges as the product's, and 1, -1 and full-width ones
    return p, rows, challenges


@pytest.mark.parametrize("fid", FIELDS)
def test_folds_preserve_the_relaxed_relation(fid):
    """Six satisfied fresh rows (az∘bz = cz, u = 1) from the value classes folded by fold_cross (the first SC elements, with the cross term it wrote at the step
    before) and fold5 (the others): AZ∘BZ = u·CZ + E after every step."""
    p, rows, ch = _chain(fid)
    assert all(x * y % p == z for az, bz, cz in rows for x, y, z in zip(az, bz, cz))
    AZ, BZ, CZ, E, u = [0] * N, [0] * N, [0] * N, [0] * N, 0
    T = [0] * N
    for i, (az, bz, cz) in enumerate(rows):
        r = ch[i]
        nxt = rows[i + 1] if i + 1 < ROWS else (None, None, None)
        head = lambda v: v[:SC] if v is not None else None
        tail = lambda v: v[SC:]
        u_new = (u + r) % p
        a, b, c, e, out, _ = fr.fold_cross(p, head(AZ), head(BZ), head(CZ), head(E), head(T), int(i > 0), r, 0, 0, None, u_new, head(az), head(bz), head(cz),
                                           i + 1 < ROWS, head(nxt[0]), head(nxt[1]), head(nxt[2]), 1, False, 0)
        f = fr.fold5(p, [(tail(AZ), tail(az)), (tail(BZ), tail(bz)), (tail(CZ), tail(cz)), (tail(E) if i else None, tail(T)), ([], [])], r)
        AZ, BZ, CZ, E, u = a + f[0], b + f[1], c + f[2], e + (f[3] if i else tail(E)), u_new
        bad = sc.unsat_rows(p, AZ, BZ, CZ, u, E)
        assert not bad, f"field {fid} step {i}: {len(bad)} elements break AZ∘BZ = u·CZ + E, first {bad[0]}"
        if i + 1 < ROWS:
            T = out + sc.cross_term(p, tail(AZ), tail(BZ), tail(CZ), u, tail(nxt[0]), tail(nxt[1]), tail(nxt[2]), 1)
    assert any(E) and u == sum(ch) % p


@pytest.mark.parametrize("fid", FIELDS)
def test_the_lookahead_identity_and_the_schedule(fid):
    """Tin − r_prev·negB with negB = fresh_cross_neg(u_prev, u) and Tin the cross term against the running instance ONE step earlier is the cross term against
    the running instance after that fold, at every step; and the schedule of launch_fold_and_cross run on the reference arrives, step by step, at the direct
    fold's AZ, BZ, CZ, E and cross terms."""
    p, rows, ch = _chain(fid)
    states = fr.direct_chain(p, rows, ch)
    zero = {"AZ": [0] * N, "BZ": [0] * N, "CZ": [0] * N, "u": 0}
    for i in range(1, ROWS):
        before = states[i - 2] if i >= 2 else zero            # the running instance that row i - 1 was folded into
        Tin = sc.cross_term(p, before["AZ"], before["BZ"], before["CZ"], before["u"], *rows[i], 1)
        negB = fr.fresh_cross_neg(p, *rows[i - 1], *rows[i])
        assert sum(1 for x in negB if x) > N // 4, (fid, i)      # the lookahead owes something at every step
        after = states[i - 1]
        assert fr.folded_vector(p, Tin, 1, ch[i - 1], negB) == sc.cross_term(p, after["AZ"], after["BZ"], after["CZ"], after["u"], *rows[i], 1) == states[i]["T"], (fid, i)
    plan = fr.schedule_plan(ROWS)
    assert [(s["fold_E"], s["hasB"], s["need1"], s["look"]) for s in plan] == [(False, False, True, True), (True, False, False, True), (True, True, False, True),
                                                                             (True, True, False, True), (True, True, False, False), (True, True, False, False)]
    steps = 0
    for st, AZ, BZ, CZ, E, t, out in fr.run_schedule(p, rows, ch, fr.fold_cross, fr.fresh_cross_neg, sc.cross_term):
        want = states[st["i"]]
        assert (AZ, BZ, CZ, E) == (want["AZ"], want["BZ"], want["CZ"], want["E"]), (fid, st)
        assert (t is None) == (out is None) == (st["i"] >= ROWS - 2)
        if t is not None:
            assert out == sc.cross_term(p, AZ, BZ, CZ, want["u"], *rows[t], 1), (fid, st)
        steps += 1
    assert steps == ROWS


@pytest.mark.parametrize("fid", FIELDS)
def test_the_cross_term_of_fold_cross_is_the_seams_and_the_oracles(oracle, fid):
    """fold_cross's out on every layout is _seam_cases.cross_term — and the oracle's — of the folded products; the masked form is the one the seam test states."""
    p = _lib.MODULUS[fid]
    assert oracle.modulus[fid] == p
    n = 333
    run = fr.running_operands(p, n, f"x:{fid}")
    cls = fr.scalar_classes(p, f"x:{fid}")
    for layout, (r, u1, u2) in zip(fr.LAYOUTS, ((cls[3], cls[4], 1), (cls[2], cls[3], cls[4]), (cls[4], cls[2], cls[3]))):
        f = fr.fresh_operands(p, layout, n, f"x:{fid}")
        a, b, c, e, out, outm = fr.fold_cross(p, run["AZ"], run["BZ"], run["CZ"], run["E"], None, 0, r, 0, 0, None, u1, f["az"], f["bz"], f["cz"], True,
                                              f["azn"], f["bzn"], f["czn"], u2, True, 37)
        assert e == run["E"] and a == [(x + r * y) % p for x, y in zip(run["AZ"], f["az"])]
        assert out == sc.cross_term(p, a, b, c, u1, f["azn"], f["bzn"], f["czn"], u2)
        got = oracle.cross_term(fid, *[sc.to_limbs(v) for v in (a, b, c)], u1, *[sc.to_limbs(f[k]) for k in ("azn", "bzn", "czn")], u2)
        assert sc.from_limbs(got) == out, (fid, layout)
        v2 = f["azn"]
        assert outm == [(2 * out[i] % p if v2[i] == 1 else 0 if v2[i] == 0 else (out[i] + a[i]) % p) if i < 37 else out[i] for i in range(n)]


def _waves(n):
    return [range(w, min(w + fr.WAVE, n)) for w in range(0, n, fr.WAVE)]


def test_the_layouts_are_what_they_claim():
    p = _lib.MODULUS[0]
    names = fr.FRESH + ("negB",)
    unit = lambda v: fr.is_unit(p, v)
    cls = lambda v: {0: 0, 1: 1, p - 1: 2, 2: 3, p - 2: 4}.get(v, 5)
    for a, b in itertools.combinations(fr.PERIODS, 2):
        assert a >= fr.FRESH_CLASSES and b >= fr.FRESH_CLASSES and math.gcd(a, b) == 1
    for n, _ in fr.sizes_and_grids():
        uni = fr.fresh_operands(p, "uniform", n, "t", names)
        gen = fr.fresh_operands(p, "generic", n, "t", names)
        cyc = fr.fresh_operands(p, "cycling", n, "t", names)
        for w in _waves(n):
            for k in names:
                assert len({uni[k][i] for i in w}) == 1 and unit(uni[k][w[0]]), (n, k)       # one class per wave and operand, none needs the multiplication
            others = [(k, i - w[0]) for k in names for i in w if not unit(gen[k][i])]
            assert len(others) == 1, (n, w, others)                                            # exactly one lane of one operand does
            assert others[0][1] == min(fr.GENERIC_LANES[(w[0] // fr.WAVE) % 4], len(w) - 1)
        if n >= 257:
            for x, y in (("az", "bzn"), ("bz", "azn")):
                assert {(cls(cyc[x][i]), cls(cyc[y][i])) for i in range(n)} == set(itertools.product(range(6), repeat=2)), (n, x, y)
            for k in names:
                assert {cls(v) for v in cyc[k]} == set(range(6))
            assert {u for k in names for u in uni[k]} == {0, 1, p - 1}
        # the vector folded into E: whole waves of zeros and waves with a single non-zero lane, with and without the lookahead's part
        if n >= 257:
            for layout, f in (("uniform", uni), ("generic", gen)):
                tin = fr.tin_vector(p, layout, n, "t")
                for hasB in (0, 1):
                    t = fr.folded_vector(p, tin, hasB, fr.scalar_classes(p, "t")[3], f["negB"])
                    nz = [sum(1 for i in w if t[i]) for w in _waves(n)]
                    assert 0 in nz and 1 in nz and max(nz) > 1, (n, layout, hasB, nz)
    run = fr.running_operands(p, 333, "t")
    assert all({cls(v) if cls(v) < 3 else 3 for v in run[k]} == {0, 1, 2, 3} for k in run)
    s = fr.scalar_classes(p, "t")
    assert s[:3] == (0, 1, p - 1) and s[3].bit_length() == 128 and s[4].bit_length() > 200


def test_the_case_lists_cover_the_options():
    """what the pruning of the k_fold_cross grid leaves (tests/_fold_ref.py: PRUNE)"""
    key = lambda o: (o["fold_E"], o["hasB"], o["out"])
    for fid in FIELDS:
        cases = fr.fold_cross_cases(fid)
        groups = {}
        for layout, n, blocks, o in cases:
            assert blocks == (1 if n == fr.STRIDED[0] else 0)
            groups.setdefault((layout, n) if fid == 0 else n, []).append(o)
        assert len(groups) == (21 if fid == 0 else 7)
        for g, opts in groups.items():
            for name, values in (("fold_E", {0, 1}), ("hasB", {0, 1}), ("out", set(fr.OUT_MODES)), ("nb", {None} | set(fr.NB)), ("u2", {0, 1}), ("r", set(range(5))),
                                 ("r_prev", set(range(5))), ("u1", set(range(5)))):
                assert {o[name] for o in opts} == values, (fid, g, name)
            if fid == 0:
                assert {key(o) for o in opts} == set(itertools.product((0, 1), (0, 1), fr.OUT_MODES)), (fid, g)
        allo = [o for opts in groups.values() for o in opts]
        assert {key(o) for o in allo} == set(itertools.product((0, 1), (0, 1), fr.OUT_MODES))
        assert {(o["out"], o["nb"]) for o in allo if o["out"] != "none"} == set(itertools.product(fr.OUT_MODES[1:], (None,) + fr.NB))
        if fid == 0:
            assert {(o["r"], o["r_prev"]) for o in allo if o["fold_E"] and o["hasB"]} == set(itertools.product(range(5), repeat=2))
    assert len(fr.fold5_cases()) == 2 * 3 * 5 * 3 and len(fr.fresh_neg_cases()) == 3 * 7 * 2
    for lens, skip, o1, o2 in fr.FOLD5_SHAPES:
        assert len(set(lens)) == 5 and 0 in lens and lens[skip] > 0 and all(o % 64 and o > 0 for o in o1 + o2)
    assert {fr.resolve_nb(s, 333) for s in fr.NB} == {0, 1, 37, 332, 333} and {fr.resolve_nb(s, 1) for s in fr.NB} == {0, 1}


@pytest.mark.parametrize("fid", FIELDS)
def test_the_raw_patterns_of_the_counting_kernels(fid):
    p = _lib.MODULUS[fid]
    pats = fr.unreduced_patterns(p)
    assert [bad for _, _, bad in pats] == [False, False, True, True, True, True, True, False, False, False]
    for name, x, bad in pats:
        assert 0 <= x < fr.R and (x >= p) == bad, name
    w = lambda x: [(x >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
    assert [a != b for a, b in zip(w(pats[5][1]), w(p))] == [True] + [False] * 7 and [a != b for a, b in zip(w(pats[6][1]), w(p))] == [False] * 7 + [True]
    cases = fr.count_cases(p, fid)
    assert {c[0] for c in cases} == {0, 1} and {c[5] for c in cases} >= {0, 1, 3, 5}
    x = cases[0][2][0]
    assert [sum(a != b for a, b in zip(w(y), w(x))) for _, y, _ in fr.diff_patterns(x)] == [1, 1, 8, 0]
