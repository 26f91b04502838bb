"""The bisection of a refused chunk in vimz_decider_verify_batch_ex, without a GPU (ctx = None: HostStages of vimz_amd/csrc/decider_batch.hpp).  Seven copies of one
of the reference's committed proofs under its key, a word changed in the first, the last, a pair in the middle, both ends and all of them; chunks of 7, 4 and 2,
leaves of 1 and 2, multipliers from the OS.  Every word is decider_verify_key's for that proof alone; the four counts are those of the planner's model
(tests/_batch_bisect_ref.py); with bisection off the words are the same, no subset equation is evaluated and every member of a refused chunk is verified singly.
Nine proofs at chunk 4 end in a chunk of ONE bad member, which goes straight to the single verifier."""
import pytest

from tests import _batch_bisect_gpu as G
from tests import _novadecider as nd
from vimz_amd.hip import decider_verify_key, verifying_key_words


@pytest.fixture(scope="module")
def matrix():
    return G.decider_matrix(None)


@pytest.fixture(scope="module")
def want():
    kw = verifying_key_words(nd.verifier_keys()["contrast"])
    good, wrong = G.decider_items()
    w = {"good": decider_verify_key(kw, *good), 0: decider_verify_key(kw, *wrong[0]), 1: decider_verify_key(kw, *wrong[1])}
    assert w["good"] == 0 and w[0] & 2 and w[1] == 8
    return lambda n, bad: [w[i % 2] if i in bad else w["good"] for i in range(n)]


@pytest.mark.parametrize("name", sorted(G.patterns(7)))
def test_words_and_counts_at_every_chunk_and_leaf(matrix, want, name):
    bad = G.patterns(7)[name]
    for chunk in G.CHUNKS:
        for leaf in G.LEAVES + ("off",):
            key = f"{name}/{chunk}/{leaf}"
            got = matrix[key]
            assert got["words"] == want(7, bad), key
            assert got["stats"] == G.decider_expected(key), key
            assert got["fallback_s"] > 0, key
        off = matrix[f"{name}/{chunk}/off"]["stats"]
        assert off[1] == 0 and off[3] == 0 and off[2] == sum(min(7, lo + chunk) - lo for lo in range(0, 7, chunk) if any(lo <= i < lo + chunk for i in bad))


def test_one_bad_member_among_seven_costs_one_single_verification(matrix):
    for name in ("first", "last"):
        for chunk in G.CHUNKS:
            refused, equations, singles, accepted = matrix[f"{name}/{chunk}/1"]["stats"]
            c = min(chunk, 7) if name == "first" else (7 - 1) % chunk + 1          # the members of the chunk the bad one is in
            assert (refused, singles, accepted) == (1, 1, c - 1) and equations <= 2 * (c - 1)


def test_a_last_chunk_of_one_bad_member_goes_straight_to_the_single_verifier(matrix, want):
    got = matrix["nine"]
    assert got["words"] == want(9, (1, 8))
    assert got["stats"] == G.decider_expected("nine") == [2, 3, 2, 3]          # the three subset equations are chunk 0's; chunk 2 asked none
    assert matrix["nine/off"]["words"] == got["words"] and matrix["nine/off"]["stats"] == [2, 0, 5, 0]


def test_the_default_leaf_gives_the_same_words(matrix, want):
    got = matrix["default_leaf"]
    assert got["words"] == want(7, (6,)) and got["stats"][0] == 1 and got["stats"][2] + got["stats"][3] == 7
