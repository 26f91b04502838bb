"""The decider's set-up from a powers-of-tau string (vimz_decider_setup_from_powers; vimz_amd/csrc/groth16.hip) and the kernels under it (g16_powers.hip:
g16_column_sums — one k_col_runs launch per level of the host plan —, g16_h_query — k_point_diff, then k_scale_points) against plain Python integers.

One probe process per part (tests/_decider_powers_gpu.py g1 | g2 | setup), so that one part's failure leaves the others' verdicts standing.  The kernels' inputs
are [s]G made by vimz_test_g16_fixed_mul (pinned on Python integers by tests/test_gpu_g16_kernels.py), the expected outputs [x]G made the same way from the
scalars tests/_g16_powers_ref.py derives; SPOT outputs of every case are compared with tests._pairing / _g16_ref.g2_gen_mul directly as well.  Every comparison is
exact equality of words.  Column sums: in G1 every case of colsum_cases() (columns of 0, 1, 31/32/33, 1 024 and 1 025 entries, the doubling pair, the cancelling
pair, cancel-then-third, the same row three times, identity rows, coefficients 1, r − 1, 2^k, r − 2^k, (r ± 1)/2, full-size and 0, at 1/63/64/65 columns and
64/empty); in G2 1/33, 65/mixed and 64/empty.  h query: n = 2, 64, 128, with delta = 1 and with an identity among the inputs.

The set-up end to end, once, on the light decider of the hash step (domain 2^18): a string of fixed (tau, alpha, beta) made on the GPU by the fixed-base hook
and passed through a `.ptau` container, set up with a fixed delta, against the trapdoor set-up with (tau, alpha, beta, gamma = 1, delta): the two saved keys
must be the same bytes; a proof under the first key must verify under vimz_decider_verify and under the restated contract (tests/_novadecider.py) with that key's
vimz_decider_vk.  Then the refusals, each with its message."""
import json
import os
import random
import subprocess
import sys

import pytest

from tests import _decider_powers_gpu as P
from tests import _g16_powers_ref as W
from tests import _g16_ref as G
from tests import _novadecider as nd
from tests._g16_kernels_gpu import hex_ints
from tests._pairing import G1, Q, R, g1_mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = 6
CASES = W.colsum_cases()


def run_probe(tmp_path_factory, what):
    out = tmp_path_factory.mktemp("decider_powers_" + what) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._decider_powers_gpu", what, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out) as fp:
        res = json.load(fp)
    res["stderr"] = r.stderr
    return res


@pytest.fixture(scope="module")
def probe_g1(tmp_path_factory):
    return run_probe(tmp_path_factory, "g1")


@pytest.fixture(scope="module")
def probe_g2(tmp_path_factory):
    return run_probe(tmp_path_factory, "g2")


@pytest.fixture(scope="module")
def probe_setup(tmp_path_factory):
    return run_probe(tmp_path_factory, "setup")


def point_words(group, s):
    """[s]G as the hooks write it"""
    if group == 1:
        p = g1_mul(G1, s % R)
        return [0, 0] if p is None else [p[0], p[1]]
    return G.g2_words(G.g2_gen_mul(s % R))


def check_colsum(probe, group, name):
    case = W.colsum_case(*CASES[name])
    want, run = W.colsum_expected(case), probe["colsum"][name]
    n, per = case["n_cols"], 2 * group
    width = 64 * per
    got, exp = run["out"], run["want"]
    assert len(got) == len(exp) == width * n
    assert got == exp, f"G{group} {name}: column {next(j for j in range(n) if got[width * j:width * j + width] != exp[width * j:width * j + width])} differs"
    words = hex_ints(got)
    assert all(c < Q for c in words)
    special = range(min(n, 12)) if group == 1 else [j for j in (3, 7, 8, 9, 10, 11) if j < n]      # the columns the mixed cases build by hand
    for j in sorted(set(special) | set(random.Random(f"colsum/spot/{group}/{name}").sample(range(n), min(n, SPOT if group == 1 else 2)))):
        assert words[per * j:per * j + per] == point_words(group, want[j]), f"G{group} {name}: column {j}"
    for j in range(n):
        assert (not any(words[per * j:per * j + per])) == (want[j] == 0), f"G{group} {name}: column {j}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_column_sums_g1(probe_g1, name):
    check_colsum(probe_g1, 1, name)


@pytest.mark.parametrize("name", P.G2_CASES)
def test_column_sums_g2(probe_g2, name):
    check_colsum(probe_g2, 2, name)


@pytest.mark.parametrize("n", P.HQ_N)
@pytest.mark.parametrize("name", ["plain", "delta_one", "identity", "identity_low"])
def test_h_query(probe_g1, n, name):
    run = probe_g1["hq"][f"{n}/{name}"]
    s, delta = P.hq_cases(n)[name]
    want = P.hq_expected(s, delta, n)
    assert run["out"] == run["want"] and len(run["out"]) == 128 * (n - 1)
    words = hex_ints(run["out"])
    for j in sorted({0, n - 2, (n - 1) // 2}):
        assert words[2 * j:2 * j + 2] == point_words(1, want[j]), f"output {j}"
    if name == "identity":
        assert want[0] == (0 - s[0]) * pow(delta, -1, R) % R and s[n] == 0
    if name == "identity_low":
        assert want[0] == s[n] * pow(delta, -1, R) % R and s[0] == 0      # the subtrahend is the identity: the minuend alone
    if name == "plain":
        assert want == [(pow(P.HQ_TAU, n, R) - 1) * pow(P.HQ_TAU, j, R) * pow(delta, -1, R) % R for j in range(n - 1)]      # Z(tau)·tau^j / delta


# ---- the set-up, end to end -------------------------------------------------------------------------------------------------------------------------------
def test_key_from_the_string_is_the_trapdoor_s_key_byte_for_byte(probe_setup):
    """Measured on one MI355X: the set-up from the string 1.7 s at this size (domain 2^18), the trapdoor set-up 0.2 s; the probe 7.9 s in all."""
    assert probe_setup["srs_is_the_strings"]
    assert probe_setup["info"] == probe_setup["info_powers"] and probe_setup["info"]["cyclefold_rows"] == 0
    key = probe_setup["key"]
    assert key["bytes"][0] == key["bytes"][1] and key["first_difference"] is None
    assert key["identical"] and key["sha256"][0] == key["sha256"][1]


def test_a_proof_under_that_key_verifies_in_the_library_and_under_the_restated_contract(probe_setup):
    pr = probe_setup["proof"]
    assert pr["verify"] == 0 and pr["verify_trapdoor_key"] == 0 and pr["verify_changed"] & 8
    from vimz_amd.hip import parse_verifying_key
    import numpy as np
    key = parse_verifying_key(np.frombuffer(bytes.fromhex(pr["key_words"]), dtype="<u8"))
    words, z0, zi = [int(w, 16) for w in pr["words"]], [int(x, 16) for x in pr["z0"]], [int(x, 16) for x in pr["z_i"]]
    # the key is the string's: alpha, beta, gamma = G2, delta of the fixed scalars
    g = key["groth16"]
    assert list(g["alpha"]) == point_words(1, P.ALPHA)
    for name, s in (("beta", P.BETA), ("gamma", 1), ("delta", P.DELTA)):
        assert [g[name][0][0], g[name][0][1], g[name][1][0], g[name][1][1]] == point_words(2, s), name
    assert [c for pair in key["kzg"]["VK"] for c in pair] == point_words(2, P.TAU)
    pub, _, _ = nd.public_inputs(key, pr["steps"], z0, zi, words)
    assert pub == [int(x, 16) for x in pr["public_inputs"]]
    assert nd.verify(key, pr["steps"], z0, zi, words) == (True, "ok")


def test_production_entry_draws_its_own_delta(probe_setup):
    od = probe_setup["os_delta"]
    assert od["verify"] == 0 and not od["same_key"] and od["verify_under_fixed_delta_key"] & 8


def test_second_call_s_seconds_and_the_plans_statistics(probe_setup):
    """The figures profiles/decider_powers.txt records: seconds[] of the second of two calls, and what the library prints under VIMZ_DECIDER_POWERS_STATS."""
    sec = probe_setup["second_call_seconds"]
    assert list(sec) == ["circuit_synthesis", "checks_and_upload", "transforms_gpu", "column_sums_gpu", "scaling_and_key_tables", "total"]
    assert all(v > 0 for v in sec.values()) and abs(sum(list(sec.values())[:5]) - sec["total"]) < 1e-6
    lines = [x for x in probe_setup["stderr"].splitlines() if x.startswith("decider from powers: ")]
    print(json.dumps(sec))
    print("\n".join(lines))
    assert len(lines) == 4                                    # one call had the switch on
    for line, plan in zip(lines, "abK"):
        assert line.startswith(f"decider from powers: plan {plan}: ") and "runs per level " in line and "level-0 runs by bitlen(|c|): 1:" in line
    assert "device memory of the set-up at its peak" in lines[3]


def test_command_line_writes_a_key_that_proves(probe_setup):
    cli = probe_setup["cli"]
    assert cli["rc"] == 0 and cli["info"] == probe_setup["info"] and cli["bytes"] == probe_setup["key"]["bytes"][0]
    assert cli["verify"] == 0 and cli["alpha_beta_gamma_are_the_strings"]


def test_e2e_tool_takes_its_keys_from_the_string(probe_setup):
    e = probe_setup["e2e"]
    assert e["rc"] == 0 and e["json"] is not None, e["stderr"]
    j = e["json"]
    assert j["verified"] and j["mode"] == "cyclefold" and j["decider"]["verified"] and j["decider"]["variant"] == "light"
    assert "column_sums_gpu" in j["decider"]["setup_s"]      # the decider came from the string, not from a trapdoor


REFUSALS = {"short_string": "shorter than the circuit's domain", "short_powers": "shorter than the circuit's domain", "not_generator": "tau_g1[0] is not the generator",
            "tau_g2_of_another_tau": "tau_g1[1] and tau_g2[1] are not of one tau", "beta_g2_of_another_beta": "beta_g1[0] and beta_g2 are not of one beta",
            "off_curve": "a point is not on its curve", "alpha_is_zero": "a point of the string is the identity", "powers_and_kzg_vk": "powers= brings its own KZG verifying key",
            "srs_of_another_tau": "the KZG verifying key is not [tau]G2 of the SRS the prover commits with"}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals(probe_setup, what):
    assert set(probe_setup["refused"]) == set(REFUSALS)
    code, message = probe_setup["refused"][what]
    assert code == probe_setup["invalid"] and REFUSALS[what] in message, (what, message)
