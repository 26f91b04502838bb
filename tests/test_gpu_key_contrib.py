"""Further delta contributions to a saved decider key on the GPU (vimz_decider_key_contribute, vimz_decider_key_verify_contributions; vimz_amd/csrc/
g16_key_contrib.hip): the new kernel through its hook, the two calls on synthetic keys, and once end to end on the light decider of the hash step.

k_ratio_rlc (one launch over both arrays, reduced by g16_column_sums over a plan of two columns) runs over tests/_key_contrib_ref.ratio_cases(): n = 1, RLC_CHUNK − 1,
RLC_CHUNK, RLC_CHUNK + 1, 19, one full wave of chunks, one point more, and 1 030 points; an identity at the same index of both arrays, a zero and an all-ones rho,
equal neighbours with equal rho (add_mixed's doubling), a chunk of opposite points that cancels, a whole sum that is the identity; "after" a true multiple of "before"
and unrelated to it.  Points are [s_i]G made by vimz_test_g16_fixed_mul (pinned on Python integers by tests/test_gpu_g16_kernels.py) and the expected sums ONE such
multiplication of Σ rho_i·s_i mod r, so every comparison is exact equality of words; SPOT sums are compared with tests._pairing directly.
The API: contribute with a fixed delta' and nonce equals the Python reference's bytes, key and record, also with key_out = key_in; chains of 0, 1 and 3 records are
accepted; every tampered chain yields exactly the bits and the first_bad the reference derives (a missed RATIO tamper has probability at most 2^-128 over the
library's rho: deterministic in practice); each refusal of contribute comes with its message.  The GPU half is tests/_key_contrib_gpu.py, a process per part."""
import json
import os
import subprocess
import sys

import pytest

from tests import _key_contrib_ref as K
from tests import _novadecider as nd
from tests._g16_kernels_gpu import hex_ints
from tests._pairing import G1, R, g1_mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = ("1/multiple", "19/unrelated", "2/whole_sum_identity")


def run_part(tmp_path_factory, part, timeout):
    out = tmp_path_factory.mktemp("key_contrib_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._key_contrib_gpu", part, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return run_part(tmp_path_factory, "kernels", 600)


@pytest.fixture(scope="module")
def api(tmp_path_factory):
    return run_part(tmp_path_factory, "api", 600)


@pytest.fixture(scope="module")
def decider(tmp_path_factory):
    return run_part(tmp_path_factory, "decider", 900)


def test_the_combination_of_two_arrays(kernels):
    cases = K.ratio_cases()
    assert set(kernels["ratio"]) == set(cases) and {len(r) for _b, _a, r in cases.values()} == set(K.RATIO_SIZES) | {2}
    for name, (before, after, rho) in cases.items():
        got = kernels["ratio"][name]
        assert got["out"] == got["want"], name
        if name in SPOT:
            s, s1 = K.ratio_scalars(before, after, rho)
            assert hex_ints(got["out"]) == list(g1_mul(G1, s) or (0, 0)) + list(g1_mul(G1, s1) or (0, 0)), name
    assert hex_ints(kernels["ratio"]["2/whole_sum_identity"]["out"]) == [0] * 4
    assert kernels["montgomery"]["out"] == kernels["montgomery"]["want"]
    assert set(kernels["bad_arguments"]) == {"n_0", "form_7", "null_after", "off_curve"} and all(rc == kernels["invalid"] for rc in kernels["bad_arguments"].values())


def test_the_two_launch_form_gives_the_same_sums(kernels):
    assert len(kernels["two_launches"]) == 3
    for name, out in kernels["two_launches"].items():
        assert out == kernels["ratio"][name]["want"], name


@pytest.mark.parametrize("name", ("small", "small_identity_in_l", "large"))
def test_contribute_equals_the_reference_byte_for_byte(api, name):
    got = api["contribute"][name]
    assert got["rc"] == got["bytes"] == got["in_place_rc"]
    assert got["key"] and got["record"], name
    assert got["in_place_key"] and got["in_place_record"], name            # key_out == key_in
    assert len(got["seconds"]) == 3 and got["seconds"][2] >= got["seconds"][1] > 0


def test_a_short_cap_returns_the_size_and_writes_nothing(api):
    sc = api["short_cap"]
    assert sc["rc"] == sc["bytes"] == sc["no_key_out"] and sc["untouched"]


@pytest.mark.parametrize("name", ("0", "1", "3", "small_identity_in_l", "null_seconds"))
def test_chains_are_accepted(api, name):
    got = api["accepted"][name]
    assert (got["rc"], got["result"], got["first_bad"]) == (0, 0, [0, 0]), name
    if name != "null_seconds":
        assert len(got["seconds"]) == 4 and all(x > 0 for x in got["seconds"]), name


@pytest.mark.parametrize("name", sorted(K.tamper_table(K.LARGE)))
def test_a_tampered_chain_yields_exactly_its_bits(api, name):
    bits, first = K.tamper_table(K.LARGE)[name]
    got = api["tampered"][name]
    assert got["rc"] == 0                                                          # a verdict, not an error
    assert (got["result"], tuple(got["first_bad"])) == (bits, first), f"{name}: 0x{got['result']:x}"


def test_the_tampers_asked_for_are_all_there():
    assert set(K.tamper_table(K.LARGE)) == {"l_h_point_scaled/first", "l_h_point_scaled/last", "l_h_point_scaled/second_chunk", "h_points_swapped", "l_point_off_curve", "coordinate_is_q",
                                            "identity_in_one_key", "a_query_byte", "record_delta2_replaced", "record_z_off_by_one", "records_swapped", "last_record_dropped"}


def test_keys_of_other_sizes(api):
    got = api["other_sizes"]
    assert (got["rc"], got["result"], got["first_bad"]) == (0, K.FIXED_PART, [K.AT_FIXED_PART, 1])


@pytest.mark.parametrize("name", K.REFUSED_KEYS)
def test_contribute_refuses_with_its_message(api, name):
    got = api["refused"][name]
    want = {"delta1_coordinate_is_q": "a coordinate is not below q", "l_coordinate_is_q": "a coordinate is not below q", "delta1_off_curve": "a delta point is not on its curve",
            "delta2_identity": "a delta point is the identity", "wrong_magic": "not a decider key", "short": "not a decider key", "odd_length": "not a decider key",
            "truncated": "wrong length", "oversized": "wrong length"}[name]
    assert got["rc"] == api["invalid"] and got["message"] == "vimz_decider_key_contribute: " + want, got


def test_bad_arguments(api):
    assert len(api["bad_arguments"]) == 14
    assert all(rc == api["invalid"] for rc in api["bad_arguments"].values()), api["bad_arguments"]
    assert api["refused_product_entry"] == api["invalid"]


def test_the_production_entry_draws_its_own_delta(api):
    od = api["os_delta"]
    assert od["rc"][0] == od["rc"][1] > 0 and od["keys_differ"] and od["records_differ"] and od["fixed_part_kept"]
    assert (od["chain"]["result"], od["first_alone"]["result"]) == (0, 0)


def test_python_and_command_line(api):
    py = api["python"]
    assert py["key"] and py["record"] and py["verify"] == [0, [0, 0]] and py["verify_bytes"] == [0, [0, 0]] and len(py["seconds"]) == 4
    assert py["tampered"] == [K.KNOWLEDGE, [K.AT_RECORD, 1]] and len(py["problems"]) == 2
    assert all(code == api["invalid"] for code, _m in py["refusals"].values()) and "wrong length" in py["refusals"]["not_a_key"][1]
    cli = api["cli"]
    assert cli["contribute_1"]["rc"] == 0 == cli["contribute_2"]["rc"] and "record 2 appended" in cli["contribute_2"]["stdout"] and cli["records_bytes"] == 2 * K.RECORD_BYTES
    assert cli["verify_2"]["rc"] == 0 and "accepted" in cli["verify_2"]["stdout"] and "after 2 contributions" in cli["verify_2"]["stdout"]
    assert cli["verify_wrong_final"]["rc"] == 1 and "REFUSED" in cli["verify_wrong_final"]["stdout"] and "last record" in cli["verify_wrong_final"]["stdout"]
    assert cli["verify_bad_key"]["rc"] == 1 and "REFUSED" in cli["verify_bad_key"]["stdout"]
    assert cli["usage_contribute"]["rc"] == 2 == cli["usage_verify"]["rc"]


# ---- end to end, once: the light decider of the hash step ------------------------------------------------------------------------------------------------
def test_a_contribution_to_the_trapdoor_key_is_the_trapdoor_key_of_the_product(decider):
    assert decider["info"]["domain"] == 1 << 18
    key = decider["key"]
    assert key["bytes"][0] == key["bytes"][1] == key["bytes"][2] and key["origin_differs"]
    assert key["identical"], f"first difference at byte {key['first_difference']}"
    info = decider["info"]
    assert key["layout"]["n_lh"] == (info["wires"] - info["public_inputs"] - 1) + (info["domain"] - 1)
    # the record, checked by the reference: the proof of knowledge over the origin's delta1, which is [delta]G1
    rec, head, before = (bytes.fromhex(decider["record"][x]) for x in ("hex", "head", "delta1_before"))
    from tests._key_contrib_gpu import DELTA
    assert K.g1_at(before, 0) == g1_mul(G1, DELTA) and K.g1_at(rec, K.REC_DELTA1) == g1_mul(G1, DELTA * K.DELTAS[0] % R)
    assert K.knowledge_holds(head, K.g1_at(before, 0), rec)
    print("vimz_decider_key_contribute on the light hash decider's key, seconds {host, device, total}:", decider["contribute_seconds"],
          "; vimz_decider_key_verify_contributions {host conversion, flags, combination, equations}:", decider["chain_seconds"])


def test_the_chain_verifies_and_a_spoiled_key_does_not(decider):
    assert decider["chain"] == [0, [0, 0]]
    assert decider["chain_without_the_record"] == [K.LAST, [0, 0]]
    assert decider["chain_two_points_swapped"] == [K.RATIO, [0, 0]]


def test_a_proof_under_the_contributed_key(decider):
    pr = decider["proof"]
    assert pr["info"] == decider["info"]
    assert pr["verify"] == 0 and pr["verify_origin_key"] == 8            # the origin key's decider refuses it: the Groth16 bit
    import numpy as np
    from vimz_amd.hip import parse_verifying_key
    key = parse_verifying_key(np.frombuffer(bytes.fromhex(pr["key_words"]), dtype="<u8"))
    words, z0, zi = [int(w, 16) for w in pr["words"]], [int(x, 16) for x in pr["z0"]], [int(x, 16) for x in pr["z_i"]]
    assert nd.verify(key, pr["steps"], z0, zi, words) == (True, "ok")


def test_the_commands_on_those_files(decider):
    cli = decider["cli"]
    assert cli["verify"]["rc"] == 0 and "accepted" in cli["verify"]["stdout"] and "after 1 contributions" in cli["verify"]["stdout"]
    assert cli["contribute"]["rc"] == 0 and "record 2 appended" in cli["contribute"]["stdout"]
    assert cli["verify_next"]["rc"] == 0 and "after 2 contributions" in cli["verify_next"]["stdout"]
    assert cli["verify_stale_final"]["rc"] == 1 and "REFUSED" in cli["verify_stale_final"]["stdout"]
