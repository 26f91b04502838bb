"""vimz_mlkzg_open end to end on the GPU (vimz_amd/csrc/mlkzg.hip) over an SRS whose tau the test chose (its powers [tau^i]G1 and [tau]G2 by the fixed-base hook, as
tests/_g16_powers_gpu.py makes them): at ℓ = 1, 2, 3, 10, 13 and n = 1, 2^ℓ − 1, 2^ℓ the commitment is vimz_msm_vec's, the evaluation and the WHOLE proof are
tests/_mlkzg_ref.py's word for word (the reference commits by one multiplication by P(tau)), hip.mlkzg_verify accepts, and after eval + 1 or a flipped word it refuses
with the bit that stage owns; every refusal of vimz_mlkzg_open.  Then one CycleFold proof over the hash step under a seeded SRS, and a merged proof of one segment:
the commitments of vimz_cf_mlkzg_open are the instance's comm_W and comm_E, the evaluations the integer multilinear evaluations of the exported running vectors, and
the verdicts 0.  The GPU half is tests/_mlkzg_gpu.py, one child process per part."""
import pytest

from tests import _mlkzg_gpu as G
from tests import _mlkzg_ref as M
from tests._g16_kernels_gpu import hex_ints
from tests._pairing import G2, g2_mul

pytestmark = pytest.mark.gpu


def _words(h):
    raw = bytes.fromhex(h)
    return [int.from_bytes(raw[i:i + 8], "little") for i in range(0, len(raw), 8)]


@pytest.fixture(scope="module")
def opened(tmp_path_factory):
    return G.run_part(tmp_path_factory, "open")


@pytest.fixture(scope="module")
def cf(tmp_path_factory):
    return G.run_part(tmp_path_factory, "cf")


def test_the_verifying_key_is_tau_g2(opened):
    assert _words(opened["vk"]) == M.g2_words(g2_mul(G2, G.TAU))


@pytest.mark.parametrize("logn", G.OPEN_LOGN)
def test_commitment_evaluation_and_proof_are_the_reference_s(opened, logn):
    x = G.point(logn)
    for n in G.open_sizes(logn):
        got = opened["open"][f"{logn}/{n}"]
        want = M.prove(G.TAU, G.coeffs(n, "open"), logn, x)
        assert got["comm"] == got["msm_vec"] and _words(got["comm"]) == want["comm"], (logn, n)
        assert got["eval"] == want["eval"], (logn, n)
        assert _words(got["proof"]) == want["proof"], (logn, n)
        assert got["verdicts"] == {"untouched": 0, "eval + 1": M.FOLD, "E_r flipped": M.FOLD, "E_r2[0] flipped": M.PAIRING, "W flipped": M.OFF_CURVE}, (logn, n)
        assert set(got["seconds"]) == {"folds", "evaluations", "divisions", "quotient_commitments"} and all(s >= 0 for s in got["seconds"].values())


def test_a_slice_of_a_longer_vector(opened):
    want = M.prove(G.TAU, G.coeffs(7, "open"), 3, G.point(3))
    assert (_words(opened["slice"]["comm"]), opened["slice"]["eval"], _words(opened["slice"]["proof"])) == (want["comm"], want["eval"], want["proof"])


def test_refusals_of_the_opening(opened):
    assert set(opened["refused"]) == {"logn_0", "logn_27", "n_0", "n_above", "past_the_vector", "srs_short", "not_fr", "not_g1", "point_r", "cap_short"}
    assert all(rc == opened["invalid"] for rc in opened["refused"].values()), opened["refused"]
    assert opened["accepted_after"] == 0


@pytest.mark.parametrize("name", ("cf", "merged"))
def test_openings_of_a_cyclefold_proof(cf, name):
    assert cf["verify"] == 0 and cf["verify_after"] == 0 and cf["merged_verify"] == 0
    got = cf[name]
    U, Z, E = hex_ints(got["instance"]), hex_ints(got["Z"]), hex_ints(got["E"])
    for which, vec, comm in ((0, Z[1:len(Z) - 2], U[0:2]), (1, E, U[2:4])):
        o = got[str(which)]
        logn = G.cf_logn(len(vec))
        x = G.point(logn, label="cf")
        assert hex_ints(o["comm"]) == comm, (name, which)
        assert o["eval"] == M.fold_levels(vec + [0] * ((1 << logn) - len(vec)), x)[logn][0], (name, which)
        assert len(_words(o["proof"])) == M.proof_words(logn)
        assert o["verdict"] == 0 and o["verdict eval + 1"] == M.FOLD, (name, which)
        assert o["refused"] == {"logn_above": cf["invalid"], "logn_below": cf["invalid"]}
