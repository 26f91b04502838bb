"""A contribution to a powers-of-tau string and the check of a chain of them on the GPU (vimz_powers_contribute, vimz_powers_verify_contributions; vimz_amd/csrc/
g16_powers_contrib.hip): the two new kernels through their hooks, the two calls on strings of known scalars, and once end to end on the light decider of the hash step.

k_power_vec runs at count = 1, 2, 3, 63, 64, 65, 129 and 1 025 (bit counts 0, 1, 2, 6, 6, 7, 8, 11; half a block, a full block, ragged blocks) for w = 1, r − 1, 2 and
a value above 2^250, against pow(w, i, r).  k_scale_points_by runs in G1 at n = 1, 63, 64, 65, 129 and in G2 at n = 1, 63, 64, 65 over tests/_powers_contrib_ref.
scale_cases(): identities at index 0 and n/2, c = 1 and random, w = 1 (the output is the input), w = r − 1 (scalars alternate between 1 and a full 254-bit walk), w
random, c = 0 (every output the identity), in place, both forms.  Points are [s_i]G made by vimz_test_g16_fixed_mul (pinned on Python integers by
tests/test_gpu_g16_kernels.py) and the expected outputs ONE such multiplication of c·w^i·s_i mod r, so every comparison is exact equality of words; SPOT cases are
compared with tests._pairing directly.
The API: contribute with fixed secrets equals the reference's string and record word for word at powers 1, 2, 3 and 7, on a prefix, with the outputs on the inputs and
in the Montgomery form; vimz_powers_verify accepts the result; chains of 0, 1 and 3 records and a chain from iden3.new_powers are accepted; every tampered chain
yields exactly the bits, the inner bits and the first_bad the reference derives (a missed string tamper has probability at most 2^-128 over the library's rho);
each refusal of contribute comes with its message.  The GPU half is tests/_powers_contrib_gpu.py, a process per part."""
import json
import os
import subprocess
import sys

import pytest

from tests import _novadecider as nd
from tests import _powers_contrib_ref as K
from tests import _powers_verify_ref as V
from tests._g16_kernels_gpu import hex_ints, ints_hex
from tests._pairing import R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = {1: ("1/w_random_c_random", "65/w_r_minus_1", "63/in_place"), 2: ("1/w_random_c_random", "63/w_r_minus_1")}
ACCEPTED = [0, 0, [0, 0]]


def run_part(tmp_path_factory, part, timeout):
    out = tmp_path_factory.mktemp("powers_contrib_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._powers_contrib_gpu", part, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
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


def verdict(got):
    return [got["result"], got["string_result"], got["first_bad"]]


@pytest.mark.parametrize("count", K.POWER_COUNTS)
def test_the_power_vector(kernels, count):
    for name, w in K.POWER_WS.items():
        assert kernels["power"][f"{count}/{name}"] == ints_hex(pow(w, i, R) for i in range(count)), name


@pytest.mark.parametrize("group", (1, 2))
def test_scaling_every_point_by_its_own_scalar(kernels, group):
    cases = K.scale_cases(group)
    got = kernels["scale"][str(group)]
    assert set(got) == set(cases) and {len(c[0]) for c in cases.values()} == set(K.SCALE_N[group])
    per = 2 * group
    for name, (s, w, c, form, _in_place) in cases.items():
        assert got[name]["out"] == got[name]["want"], name
        assert got[name]["input_kept"], name
        n = len(s)
        if name.endswith("/w_one_c_one"):
            assert got[name]["out"] == got[name]["input"], name                     # the output IS the input
        if name.endswith("/c_zero"):
            assert hex_ints(got[name]["out"]) == [0] * (per * n), name               # every output the identity
        out = hex_ints(got[name]["out"])
        for i in {0, n // 2}:
            assert out[per * i:per * i + per] == [0] * per, name                     # the identity stays the identity
        if name in SPOT[group]:
            assert form == "canonical"
            want = [x for e in K.scale_expected(s, w, c) for x in V.flat(group, V.mul(group, e))]
            assert out == want, name
    assert set(kernels["bad_arguments"]) == {"n_0", "group_3", "form_7", "null_out", "w_is_r", "off_curve", "power_count_0", "power_w_is_r"}
    assert all(rc == kernels["invalid"] for rc in kernels["bad_arguments"].values()), kernels["bad_arguments"]


@pytest.mark.parametrize("power", K.POWERS)
def test_contribute_equals_the_reference_word_for_word(api, power):
    got = api["contribute"][str(power)]
    assert got["n_tau_g1"] == 2 * (1 << power) - 1
    assert got["rc"] == 0 == got["in_place_rc"]
    assert got["points"] and got["record"] and got["differs"], power
    assert got["in_place_points"] and got["in_place_record"], power                  # the outputs on the inputs
    assert len(got["seconds"]) == 3 and got["seconds"][2] >= got["seconds"][1] > 0
    assert got["powers_verify"] == [0, 0, [0, 0]]                                    # vimz_powers_verify accepts the result


def test_the_smallest_string_against_the_pairing_module(api):
    s0, s1 = K.chain_scalars(1, 1)
    want, rec = K.contribute_points(V.string_points(s0), K.SECRET_SETS[0], K.NONCE_SETS[0])
    for name in V.ARRAYS[1:]:
        assert hex_ints(api["spot"]["out"][name]) == [c for p in want[name] for c in V.flat(V.GROUP[name], p)], name
    assert api["spot"]["record"] == rec.hex()


def test_a_prefix_and_the_montgomery_form(api):
    assert api["prefix"] == {"rc": 0, "points": True, "record": True}                # n_tau_g1 = n_pow
    assert api["montgomery"] == {"rc": 0, "points": True, "record": True}


@pytest.mark.parametrize("name", (f"{K.TAMPER_POWER}/0", f"{K.TAMPER_POWER}/1", f"{K.TAMPER_POWER}/3", "7/3", "null_seconds", "montgomery"))
def test_chains_are_accepted(api, name):
    got = api["accepted"][name]
    assert got["rc"] == 0 and verdict(got) == ACCEPTED, name
    if name != "null_seconds":
        assert len(got["seconds"]) == 3 and got["seconds"][2] > 0, name


def test_a_chain_from_the_new_string(api):
    new = api["new"]
    assert new["points"] and new["record"]
    assert new["chain"] == ACCEPTED and new["first_alone"] == ACCEPTED and new["no_records"] == ACCEPTED
    assert new["second_without_first"] == [K.KNOWLEDGE_ALL, 0, [K.AT_RECORD, 0]]
    assert new["powers_verify"] == [0, [0, 0]]


@pytest.mark.parametrize("name", sorted(K.tamper_table()))
def test_a_tampered_chain_yields_exactly_its_bits(api, name):
    bits, sbits, first = K.tamper_table()[name]
    got = api["tampered"][name]
    assert got["rc"] == 0                                                            # a verdict, not an error
    assert (got["result"], got["string_result"], tuple(got["first_bad"])) == (bits, sbits, first), f"{name}: 0x{got['result']:x} 0x{got['string_result']:x}"


def test_the_tampers_asked_for_are_all_there():
    assert set(K.tamper_table()) == ({f"record_{part}/{s}" for part in "ATz" for s in K.SECRETS} | {f"final_point/{a}" for a in V.ARRAYS[1:]}
                                     | {"records_swapped", "last_record_dropped", "middle_record_dropped", "last_record_of_another_string", "final_point_off_curve",
                                        "record_point_identity", "record_point_off_curve", "origin_coordinate_is_q"})


@pytest.mark.parametrize("name", sorted(K.REFUSED_STRINGS))
def test_contribute_refuses_with_its_message(api, name):
    got = api["refused"][name]
    assert got["rc"] == api["invalid"] and got["message"] == "vimz_powers_contribute: " + K.REFUSED_STRINGS[name], got
    assert got["untouched"]                                                          # nothing is written unless everything succeeded


def test_bad_arguments(api):
    assert len(api["bad_arguments"]) == 3 + 10 + 6 + 11 + 3
    assert all(rc == api["invalid"] for rc in api["bad_arguments"].values()), api["bad_arguments"]
    assert api["refused_product_entry"] == api["invalid"]
    assert api["bad_messages"]["record_magic"] == "vimz_powers_verify_contributions: record 1: not a contribution record"
    assert api["bad_messages"]["n_pow_1"] == "vimz_powers_contribute: needs n_pow >= 2 and n_tau_g1 >= n_pow"


def test_the_production_entry_draws_its_own_secrets(api):
    got = api["os_secrets"]
    assert got["rc"] == [0, 0, 0] and got["strings_differ"] and got["records_differ"] and got["generators_kept"]
    assert verdict(got["chain"]) == ACCEPTED and verdict(got["first_alone"]) == ACCEPTED
    assert verdict(got["other_first"]) == [K.KNOWLEDGE_ALL, 0, [K.AT_RECORD, 1]]     # a record made over another contributor's string


def test_python_and_command_line(api):
    py = api["python"]
    assert py["points"] and py["record"] and py["power"] == K.TAMPER_POWER and py["round_trip"] and len(py["seconds"]) == 3 and len(py["verify_seconds"]) == 3
    assert py["verify"] == ACCEPTED and py["verify_points"] == ACCEPTED and py["verify_words"] == ACCEPTED
    assert py["tampered"] == [K.KNOWLEDGE_ALPHA, 0, [K.AT_RECORD, 1]] and len(py["problems"]) == 2
    assert all(code == api["invalid"] for code, _m in py["refusals"].values()), py["refusals"]
    assert "not on its curve" in py["refusals"]["off_curve"][1] and "488" in py["refusals"]["records_length"][1]
    cli = api["cli"]
    assert cli["new"]["rc"] == 0 and cli["origin_is_new_powers"]
    assert cli["contribute_1"]["rc"] == 0 == cli["contribute_2"]["rc"] and "record 2 appended" in cli["contribute_2"]["stdout"] and cli["records_bytes"] == 2 * K.RECORD_BYTES
    assert cli["verify_2"]["rc"] == 0 and "accepted" in cli["verify_2"]["stdout"] and "after 2 contributions" in cli["verify_2"]["stdout"]
    assert cli["verify_wrong_final"]["rc"] == 1 and "REFUSED" in cli["verify_wrong_final"]["stdout"] and "LAST" in cli["verify_wrong_final"]["stdout"]
    assert cli["usage_new"]["rc"] == 2 == cli["usage_contribute"]["rc"] == cli["usage_verify"]["rc"]


# ---- end to end, once: the light decider of the hash step ------------------------------------------------------------------------------------------------
def test_a_decider_key_from_a_string_contributed_to(decider):
    assert decider["info"]["domain"] == 1 << 18
    assert decider["record_bytes"] == K.RECORD_BYTES and decider["string_changed"]
    assert decider["chain"] == ACCEPTED
    assert decider["chain_without_the_record"] == [K.LAST, 0, [0, 0]]
    pr = decider["proof"]
    assert pr["kzg_vk_is_the_contributed_strings"] and pr["kzg_vk_is_not_the_origins"]
    assert pr["verify"] == 0                                                         # vimz_decider_verify
    import numpy as np
    from vimz_amd.hip import parse_verifying_key
    key = parse_verifying_key(np.frombuffer(bytes.fromhex(pr["key_words"]), dtype="<u8"))
    words, z0, zi = [int(w, 16) for w in pr["words"]], [int(x, 16) for x in pr["z0"]], [int(x, 16) for x in pr["z_i"]]
    assert nd.verify(key, pr["steps"], z0, zi, words) == (True, "ok")                # the restated contract
    print("vimz_powers_contribute on a string of power 18, seconds {host, device, total}:", decider["contribute_seconds"],
          "; vimz_powers_verify_contributions {points, knowledge, string}:", decider["chain_seconds"])
