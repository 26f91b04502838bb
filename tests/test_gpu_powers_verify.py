"""Judging a powers-of-tau string on the GPU (vimz_powers_verify; vimz_amd/csrc/g16_powers_verify.hip): the kernels through their hooks, the verdicts, and the
calls that take the new flag.

The combination (k_powers_rlc twice, each reduced by g16_column_sums) and the per-point flags (k_powers_flags) run over the cases of tests/_powers_verify_ref.py —
the sizes around a chunk of RLC_CHUNK pairs and around a block of 64 chunks, zero / one / 2^128 − 1 / single / random scalars, chunk sums that are equal and opposite; one
bad point of every kind at the first, the middle and the last index of 63, 64 and 65 points.  Points are [s_i]G made by vimz_test_g16_fixed_mul (pinned on Python
integers by tests/test_gpu_g16_kernels.py) and the expected sums ONE such multiplication of Σ rho_i·s_i mod r, so every comparison is exact equality of words; SPOT
sums are compared with tests._pairing directly.  vimz_powers_verify accepts good strings and refuses, with exactly the bits that follow from its equations and the
place of the first per-point finding, strings with one thing wrong.  The GPU half is tests/_powers_verify_gpu.py, a process per part."""
import json
import os
import subprocess
import sys

import pytest

from tests import _powers_verify_gpu as P
from tests import _powers_verify_ref as V
from tests._g16_kernels_gpu import hex_ints

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = ("1/random", f"{V.RLC_CHUNK + 1}/opposite", f"{V.RLC_CHUNK + 1}/max")


def run_part(tmp_path_factory, part, timeout):
    out = tmp_path_factory.mktemp("powers_verify_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._powers_verify_gpu", part, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
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


@pytest.mark.parametrize("group", (1, 2))
def test_the_combination(kernels, group):
    cases = V.rlc_cases(group)
    assert {k for k in kernels["rlc"] if k.startswith(f"{group}/")} == {f"{group}/{name}" for name in cases}
    s = V.base_scalars()
    for name, rho in cases.items():
        got = kernels["rlc"][f"{group}/{name}"]
        assert got["out"] == got["want"], f"G{group} {name}"
        if name.endswith("/zero"):
            assert hex_ints(got["out"]) == [0] * (4 * group), name               # S and S' are the identity
        if name in SPOT:
            want = V.rlc_scalars(s, rho)
            assert hex_ints(got["out"]) == V.flat(group, V.mul(group, want[0])) + V.flat(group, V.mul(group, want[1])), name


def test_the_cases_reach_the_reductions_branches():
    s = V.base_scalars()
    for group in (1, 2):
        cases = V.rlc_cases(group)
        big = max(V.RLC_PAIRS[group])
        c = V.rlc_chunk_scalars(s, cases[f"{big}/opposite"], 0)
        assert len(c) == V.PT_BLOCK + 1 and c[0] and (c[0] + c[1]) % V.R == 0 and c[-1] and not any(c[2:-1])      # cancellation, then a restart
        c = V.rlc_chunk_scalars(s, cases[f"{big}/equal"], 0)
        assert c[1] and c[1] == c[2] and not c[0] and not any(c[3:])                                            # a doubling


@pytest.mark.parametrize("group", (1, 2))
def test_the_flags(kernels, group):
    kinds = V.bad_points(group)
    cases = V.flags_cases(group)
    assert {k for k in kernels["flags"] if k.startswith(f"{group}/")} == {f"{group}/{name}" for name in cases}
    for name, (s, bad) in cases.items():
        want = [kinds[bad[i]][1] if i in bad else 0 for i in range(len(s))]
        assert kernels["flags"][f"{group}/{name}"] == want, f"G{group} {name}"


def test_good_strings_are_accepted(api):
    for name, got in api["accepted"].items():
        assert (got["rc"], got["result"], got["first_bad"]) == (0, 0, [0, 0]), name
        assert len(got["seconds"]) == 4 and all(x > 0 for x in got["seconds"]), name
    assert (api["null_seconds"]["rc"], api["null_seconds"]["result"]) == (0, 0)
    assert (api["beyond_the_prefix"]["rc"], api["beyond_the_prefix"]["result"]) == (0, 0)


@pytest.mark.parametrize("name", sorted(P.refused_cases()))
def test_a_bad_string_is_refused_with_its_bits(api, name):
    _change, bits, first = P.refused_cases()[name]
    got = api["refused"][name]
    assert got["rc"] == 0                                                          # a verdict, not an error
    assert (got["result"], tuple(got["first_bad"])) == (bits, first), f"{name}: 0x{got['result']:x}"


def test_the_first_array_with_a_finding_is_named(api):
    got = api["two_findings"]
    assert (got["rc"], got["result"], got["first_bad"]) == (0, V.IDENTITY, [2, 5])


def test_bad_arguments(api):
    assert len(api["bad_arguments"]) == 11
    assert all(rc == api["invalid"] for rc in api["bad_arguments"].values()), api["bad_arguments"]


def test_python_and_command_line(api):
    py = api["python"]
    assert py["whole"] == [0, [0, 0]] and py["n_8"] == [0, [0, 0]] and len(py["seconds"]) == 4
    assert py["mixed"] == [V.SUBGROUP, [2, P.MID]] and py["mixed_beyond_n_8"] == [0, [0, 0]]
    assert py["refusals"] == {"n_1": api["invalid"], "n_above": api["invalid"]}
    cli = api["cli"]
    assert cli["good"]["rc"] == 0 and "accepted" in cli["good"]["stdout"] and "pairings" in cli["good"]["stdout"]
    assert cli["good_8"]["rc"] == 0 and "8 points (tau_g1: 15)" in cli["good_8"]["stdout"]
    assert cli["bad"]["rc"] == 1 and "REFUSED" in cli["bad"]["stdout"] and f"tau_g2[{P.MID}]" in cli["bad"]["stdout"] and "outside the subgroup" in cli["bad"]["stdout"]
    assert cli["usage"]["rc"] == 2


def test_the_decider_judges_the_string_only_when_asked(decider):
    inv = decider["invalid"]
    n = decider["domain"]
    assert n == 1 << 18
    assert decider["good_verified"]["code"] == 0 and decider["verdict"] == [0, [0, 0]]
    print("vimz_powers_verify over the light hash decider's prefix, seconds {host conversion, flags, combinations, pairings}:", decider["verdict_seconds"],
          "; Decider(verify_powers=True) in all:", decider["good_verified"]["seconds"], "of which the set-up", decider["good_verified"]["setup_seconds"]["total"])
    assert decider["bad_verdict"] == [V.RATIO_TAU_G1, [0, 0]]
    bad = decider["bad_verified"]
    assert bad["code"] == inv and "tau_g1 is not the powers of one tau" in bad["message"] and "Decider" in bad["message"]
    assert decider["bad_default"]["code"] == 0 and decider["bad_default"]["info"] == decider["good_verified"]["info"]      # as before: nobody looks
    assert decider["kzg_bad_verified"]["code"] == inv and "kzg_from_powers" in decider["kzg_bad_verified"]["message"]
    assert decider["kzg_bad_default"]["code"] == 0
    assert decider["flag_without_powers"]["code"] == inv
