"""The bisection of a refused chunk in the batched compressed-proof verifier on the GPU (vimz_amd/csrc/spartan_batch.hpp: compressed_batch asks batch_side_equation
again of halves of the chunk — k_svec_accum and the two msm_run calls over the arguments of a subset, every opening under the multiplier it had).

On a caller's instances (vimz_test_spartan_instance_batch_ex, the smallest shapes of tests/_spartan_batch_gpu.py, both curves): 5, 7 and 8 members, chunks of 32, 4
and 2, leaves of 1 and 2, wrong-W and wrong-E members mixed at the first place, the last, a pair in the middle, both ends and everywhere; multipliers from the OS,
and again with fixed non-trivial 128-bit ones (never all ones: whoever knows the multipliers can make wrong members cancel).  Every result is the single instance
verifier's for that member; the four counts are the planner model's (tests/_batch_bisect_ref.py).
End to end on `hash` at HD: six Nova + CycleFold proofs, member 1 with only its Grumpkin argument wrong, member 4 with only a BN254 argument wrong.  The words are
the single verifier's, and the count of side equations shows that no subset was asked on a curve that held for its parent (the test's docstring has why the
BN254-wrong member never reaches a chunk; subsets refused on both curves are the planner tests', tests/test_batch_bisect_*_host.py).
The GPU half is tests/_batch_bisect_gpu.py, a process a part."""
import pytest

from tests import _batch_bisect_gpu as G
from tests import _batch_bisect_ref as R
from tests.test_gpu_decider_batch_bisect import run_part

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def instance(tmp_path_factory):
    return run_part(tmp_path_factory, "instance", 900)


@pytest.fixture(scope="module")
def cf(tmp_path_factory):
    return run_part(tmp_path_factory, "cf", 900)["cf"]


@pytest.mark.parametrize("n", G.INSTANCE_N)
@pytest.mark.parametrize("cid", (0, 1))
def test_instances_at_every_chunk_and_leaf(instance, cid, n):
    r = instance[str(cid)]
    assert r["single"] == {"good": 1, "W": 0, "E": 0}
    seen = 0
    for name, bad in G.patterns(n).items():
        want = [0 if i in bad else 1 for i in range(n)]
        for chunk in G.INSTANCE_CHUNKS:
            for leaf in G.LEAVES + ("off",):
                key = f"{n}/{name}/{chunk}/{leaf}"
                for source in ("os", "fixed") if leaf != "off" else ("os",):
                    got = r[source][key]
                    print(cid, source, key, got)
                    assert got["results"] == want, (cid, source, key)
                    assert got["stats"] == G.instance_expected(cid, n, name, chunk, leaf), (cid, source, key)
                    assert got["fallback_s"] > 0
                    seen += 1
    assert seen == 5 * 3 * 5


def test_one_bad_member_of_eight_costs_three_to_six_equations_and_one_single_verification(instance):
    for cid in (0, 1):
        for name in ("first", "last"):
            refused, equations, singles, accepted = instance[str(cid)]["os"][f"8/{name}/0/1"]["stats"]
            assert (refused, singles, accepted) == (1, 1, 7) and 3 <= equations <= 6
        assert instance[str(cid)]["os"]["8/first/0/off"]["stats"] == [1, 0, 8, 0]


def test_six_cyclefold_proofs_each_half_wrong_on_one_curve(cf):
    """Member 1 (first half) has a bit of its Grumpkin argument flipped, member 4 (second half) a bit of its last BN254 argument.  A proof's three arguments share
    ONE transcript (running | fresh | cyclefold, the Grumpkin one last), so the flipped BN254 scalar changes the challenges of the Grumpkin argument after it: the
    deferred replay of member 4 fails there on the host, and the member leaves for the single verifier BEFORE the chunk is formed, as every member with a failed
    deferred pass does.  (The single verifier stops at the BN254 argument: its word has that bit alone.)  The chunk is therefore the other five members, refused on
    the Grumpkin curve alone, and the counts are the model's for five members with member 1 bad on side 2, plus member 4's single verification.  BN254 held for the
    chunk and is never asked again: every subset costs ONE side equation."""
    assert [w == 0 for w in cf["single"]] == [i not in G.CF_BAD for i in range(6)]
    assert cf["single"][1] != cf["single"][4]                                     # the two wrong members fail on different arguments
    for name in ("leaf1", "default", "off"):
        assert cf[name]["words"] == cf["single"], name
    print(cf)
    model = R.plan([(0, 5)], {1: 2}, 1)
    refused, equations, singles, accepted = model["stats"]
    assert all(sides == 2 for _, _, sides in model["asked"]) and equations == model["subsets"]          # one curve a subset
    want = [refused, equations, singles + 1, accepted]
    assert cf["leaf1"]["stats"] == want == cf["default"]["stats"]          # (the default leaf of the compressed verifiers is 1)
    assert want == [1, 5, 2, 4]
    assert cf["off"]["stats"] == [1, 0, 6, 0]
    assert cf["leaf1"]["fallback_s"] < cf["off"]["fallback_s"]              # two single verifications and five side equations against six single verifications
    assert cf["folding"]["words"] == cf["single"] and cf["folding"]["stats"] == dict(zip(("chunks_refused", "subset_equations", "single_verifications", "accepted_by_subset"), want))
