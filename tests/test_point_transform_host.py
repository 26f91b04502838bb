"""The point transform of a set-up from a powers-of-tau string (vimz_amd/csrc/g16_powers.hip) without a GPU.

The algorithm: tests/native/pt_stage_check.cpp loops the functions the kernels call with their thread index (vimz_amd/csrc/g16_point_stage.hpp) over every
index of every launch on the CPU, built with g++ -fsanitize=address,undefined and run directly.  Its outputs are compared here, word for word, with
[s]G of the scalars tests/_g16_powers_ref.transform_expected gives (tests._pairing.g1_mul, _g16_ref.g2_gen_mul): every case forward, `random` and `holes` in every
direction — every output up to logn 3; at logn 6 SPOT outputs of every run (a scalar multiplication in Python integers takes 80 ms), and in full what needs
none: forward and back is the input, e_0 gives n generators, identities stay identities.  G1 at logn 1, 2, 3, 6, G2 at 1, 2, 3.

The refusals of hip.lagrange_from_powers that need no device, over strings written by tests/test_ptau_host.write_ptau at powers 1 and 2."""
import os
import random
import subprocess

import pytest

from tests import _g16_powers_ref as W
from tests import _g16_ref as G
from tests._pairing import G1, g1_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_LOGN = {1: (1, 2, 3, 6), 2: (1, 2, 3)}
OPS = {"fwd": "f", "inv": "i", "inv_scaled": "I", "back_unscaled": "fi", "back": "fI", "in": "n"}      # transform_expected's runs as pt_stage_check's OPS; the input
SPOT = 8                         # outputs of a run above that size compared with g1_mul


def runs():
    """label -> (group, logn, ops, input scalars, expected scalars)"""
    out = {}
    for group, logns in NATIVE_LOGN.items():
        for logn in logns:
            for name, s in W.transform_cases(logn).items():
                want = W.transform_expected(s, logn, name)
                for what, x in {**want, **({"in": s} if "back" in want else {})}.items():
                    out[f"{group}/{logn}/{name}/{what}"] = (group, logn, OPS[what], s, x)
    return out


RUNS = runs()


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("pt_stage")
    exe, spec = d / "pt_stage_check", d / "runs.txt"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "pt_stage_check.cpp")])
    spec.write_text("".join(f"{label} {g} {logn} {ops} " + " ".join(f"{x:x}" for x in s) + "\n" for label, (g, logn, ops, s, _) in RUNS.items()))
    out = subprocess.run([str(exe), str(spec)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = {}
    for line in out.stdout.splitlines():
        label, *words = line.split()
        assert label not in lines
        lines[label] = [int(w, 16) for w in words]
    return lines


@pytest.fixture(scope="module")
def point_of():
    """scalar -> the words of [s]G, each computed once"""
    memo = {1: {}, 2: {}}

    def words(group, s):
        if s not in memo[group]:
            p = g1_mul(G1, s) if group == 1 else G.g2_gen_mul(s)
            memo[group][s] = ([0, 0] if p is None else list(p)) if group == 1 else G.g2_words(p)
        return memo[group][s]
    return words


def test_every_run_is_reported(native):
    assert set(native) == set(RUNS)


@pytest.mark.parametrize("label", sorted(RUNS))
def test_cpu_loop_of_the_kernels_functions(native, point_of, label):
    group, logn, _, _, want = RUNS[label]
    per = 2 * group
    got = native[label]
    assert len(got) == per << logn
    n = 1 << logn
    spot = range(n) if n <= SPOT else sorted({0, 1, n // 2, n - 1} | set(random.Random("pt_stage/spot/" + label).sample(range(n), SPOT - 4)))
    for j in spot:
        assert got[per * j:per * j + per] == point_of(group, want[j]), f"{label}: output {j}"
    if label.endswith("/back"):
        assert got == native[label[:-4] + "in"]                  # forward, then the scaled inverse: the input, every point of it
    if label.endswith(("/e_0/fwd", "/identity/fwd")):
        assert got == point_of(group, want[0]) * n               # n generators; n identities


def test_the_cases_reach_what_they_are_meant_to():
    for group, logns in NATIVE_LOGN.items():
        assert set(logns) <= set(W.TRANSFORM_LOGN[group])
    s = W.transform_cases(3)
    assert s["half_period"][:4] == s["half_period"][4:] and 0 in s["holes"] and not any(s["identity"])
    e0 = W.transform_expected(s["e_0"], 3, "e_0")["fwd"]
    assert e0 == [1] * 8                                   # n copies of the generator
    assert set(W.transform_expected(s["random"], 3)) | {"in"} == set(OPS)


# ---- hip.lagrange_from_powers: the refusals that need no device ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def powers():
    from tests.test_ptau_host import string_of, write_ptau
    from vimz_amd import iden3
    return {p: iden3.read_ptau(write_ptau(p, string_of(p))) for p in (1, 2)}


class NoDevice:
    """stands where a Context would: any use of it is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"lagrange_from_powers touched the context ({name}) before refusing")


@pytest.mark.parametrize("power", [1, 2])
def test_lagrange_from_powers_refuses_without_a_device(powers, power):
    from vimz_amd import _lib, hip
    pw = powers[power]
    n2 = 1 << power
    bad = [(pw, power + 1), (pw, 0), (pw, -1)]
    for name in ("tau_g1", "alpha_g1", "beta_g1", "tau_g2"):
        bad.append((dict(pw, **{name: pw[name][:n2 - 1]}), power))
    for string, logn in bad:
        with pytest.raises(_lib.VimzError) as e:
            hip.lagrange_from_powers(NoDevice(), string, logn)
        assert e.value.code == _lib.ERR_INVALID


def test_command_line_form_states_its_usage(capsys):
    from vimz_amd import iden3
    assert iden3._main(["lagrange", "only.ptau"]) == 2 and iden3._main(["other", "a", "1", "b"]) == 2
    assert "lagrange FILE.ptau LOGN OUT.npz" in capsys.readouterr().err
