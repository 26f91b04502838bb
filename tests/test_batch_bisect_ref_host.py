"""tests/_batch_bisect_ref.py — the model of the batch verifiers' bisection planner (vimz_amd/csrc/batch_bisect.hpp) — against the properties the planner is
wanted for, over EVERY bad subset of c = 1…9 members at leaf 1…4, with one side and with two.  No GPU."""
import pytest

from tests import _batch_bisect_ref as B

SIDE_PATTERNS = (lambda i: 1, lambda i: 1 + (i & 1), lambda i: i % 3 + 1)


def cases(c):
    for pattern, side in enumerate(SIDE_PATTERNS):
        for badset in range(1 << c):
            yield pattern, badset, {i: side(i) for i in range(c) if (badset >> i) & 1}


@pytest.mark.parametrize("c", range(1, 10))
@pytest.mark.parametrize("leaf", (1, 2, 3, 4))
def test_every_member_is_judged_once_and_soundly(c, leaf):
    for _, badset, bad in cases(c):
        got = B.plan([(0, c)], bad, leaf)
        refused_sides = 0
        for m in bad.values():
            refused_sides |= m
        single = [i for lo, hi, _ in got["singles"] for i in range(lo, hi)]
        assert len(single) == len(set(single))
        # an accepted subset: asked, and no member of it fails on a side it was asked on
        clean = [(lo, hi, s) for lo, hi, s in got["asked"] if not any(bad.get(i, 0) & s for i in range(lo, hi))]
        held = {i for lo, hi, _ in clean for i in range(lo, hi)}
        for i in range(c):
            if i in bad:
                assert i in single and i not in held, (c, leaf, badset, i)          # every bad member is judged singly, never accepted by a subset
            elif bad:
                assert (i in single) != (i in held), (c, leaf, badset, i)            # every other one: in a subset that held, or before the single verifier; not both
        if not bad:
            assert got == {"asked": [], "singles": [], "subsets": 0, "stats": [0, 0, 0, 0]}
            continue
        if leaf == 1:
            assert sorted(single) == sorted(bad)
        # no side that held for a parent is asked again: a subset is asked only on sides on which the chunk and every asked subset around it failed
        for lo, hi, s in got["asked"]:
            assert s and not s & ~refused_sides
            for lo2, hi2, s2 in got["asked"]:
                if lo2 <= lo and hi <= hi2 and (lo2, hi2) != (lo, hi):
                    failed = 0
                    for i in range(lo2, hi2):
                        failed |= bad.get(i, 0)
                    assert not s & ~(s2 & failed), (c, leaf, badset, (lo, hi, s), (lo2, hi2, s2))
        assert got["subsets"] <= 2 * (c - 1), (c, leaf, badset)
        assert got["stats"] == [1, sum(bin(s).count("1") for _, _, s in got["asked"]), len(single), len(held - set(single))]
        assert got["stats"][2] + got["stats"][3] == c
        if c <= leaf:
            assert got["asked"] == [] and got["singles"] == [(0, c, refused_sides)]


def test_one_bad_member_among_a_power_of_two_costs_between_k_and_2k():
    for k in range(1, 7):
        c = 1 << k
        seen = set()
        for at in range(c):
            got = B.plan([(0, c)], {at: 1}, 1)
            assert k <= got["subsets"] <= 2 * k and got["stats"] == [1, got["subsets"], 1, c - 1], (k, at)
            seen.add(got["subsets"])
        assert seen == set(range(k, 2 * k + 1))          # the last member costs k (every L holds, every R is implied), the first 2k, and everything between occurs


def test_a_chunk_bad_throughout_meets_the_bound():
    for c in range(2, 33):
        got = B.plan([(0, c)], {i: 1 for i in range(c)}, 1)
        assert got["subsets"] == 2 * (c - 1) and got["stats"] == [1, 2 * (c - 1), c, 0]


def test_chunks_are_levelled_together_and_clean_chunks_take_no_part():
    roots = B.chunks_of(9, 4)
    got = B.plan(roots, {1: 1, 8: 1}, 1)
    # level 1: the L of chunk 0 ([0, 2) refused), then its R; chunk 2 is one member: straight to the single verifier.  Level 2: [0, 1) holds, so [1, 2) is implied
    assert got["asked"] == [(0, 2, 1), (2, 4, 1), (0, 1, 1)] and got["singles"] == [(8, 9, 1), (1, 2, 1)] and got["stats"] == [2, 3, 2, 3]
    assert B.stats_without_bisection(roots, {1: 1, 8: 1}) == [2, 0, 5, 0]
    # two sides: each half is asked further only on the side it failed on
    got = B.plan([(0, 6)], {1: 2, 4: 1}, 1)
    assert got["asked"][:2] == [(0, 3, 3), (3, 6, 3)] and all(s == (2 if hi <= 3 else 1) for lo, hi, s in got["asked"][2:])
    assert got["stats"] == [1, 4 + len(got["asked"]) - 2, 2, 4]
