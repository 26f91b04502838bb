"""The kernels of vimz_powers_verify (vimz_amd/csrc/g16_powers_verify.hip: k_powers_flags, k_powers_rlc and the reduction of its chunk sums) without a GPU.

tests/native/pt_verify_check.cpp, built with g++ -fsanitize=address,undefined and run directly, loops the functions the kernels call with their thread index
(g16_point_stage.hpp: pt_flags, pt_rlc_chunk, colsum_run over rlc_sum_plan's plan) over every thread of every launch, in G1 and in G2, for the cases of
tests/_powers_verify_ref.py — the sizes around a chunk and around a block of chunks, zero / one / 2^128 − 1 / single / random scalars, chunk sums that are equal
and that are opposite; one bad point of every kind the device judges at the first, the middle and the last index.  Here its words against the Python reference:
S, S' and SPOT chunk sums of every case as [Σ rho·s]G on integers, every flag."""
import os
import random
import subprocess

import pytest

from tests import _powers_verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = 2
RLC = {group: V.rlc_cases(group) for group in (1, 2)}
FLAGS = {group: V.flags_cases(group) for group in (1, 2)}
HOST_KINDS = {"x_is_q"}      # the coordinates' range is the host's conversion, not pt_flags': the program gets a good point there


def flags_tokens(group, s, bad):
    kinds = V.bad_points(group)
    tok = []
    for i, x in enumerate(s):
        if i in bad and bad[i] not in HOST_KINDS:
            tok.append("p:" + ",".join(f"{c:x}" for c in V.flat(group, kinds[bad[i]][0])))
        else:
            tok.append(f"s:{x:x}")
    return " ".join(tok)


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("pt_verify")
    exe, spec = d / "pt_verify_check", d / "cases.txt"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "pt_verify_check.cpp")])
    lines = []
    for group in (1, 2):
        lines.append(V.base_line(group))
        lines += [f"RLC rlc/{group}/{name} {group} {len(rho)} " + " ".join(f"{x:x}" for x in rho) for name, rho in RLC[group].items()]
        lines += [f"FLAGS flags/{group}/{name} {group} " + flags_tokens(group, s, bad) for name, (s, bad) in FLAGS[group].items()]
    spec.write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(spec)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = {}
    for line in out.stdout.splitlines():
        label, *words = line.split()
        res[label] = [int(w, 16) for w in words] if label.startswith("rlc/") else [int(w) for w in words]
    return res


def test_every_case_is_reported(native):
    assert set(native) == {f"rlc/{g}/{name}" for g in (1, 2) for name in RLC[g]} | {f"flags/{g}/{name}" for g in (1, 2) for name in FLAGS[g]}


@pytest.mark.parametrize("group", (1, 2))
def test_cpu_loop_of_the_combination(native, group):
    s, per = V.base_scalars(), 2 * group
    for name, rho in RLC[group].items():
        got = native[f"rlc/{group}/{name}"]
        chunks = V.rlc_chunk_scalars(s, rho, 0)
        assert len(got) == per * (2 + len(chunks)), name
        point = lambda k: got[per * k:per * k + per]      # noqa: E731
        want = V.rlc_scalars(s, rho)
        assert point(0) == V.flat(group, V.mul(group, want[0])), f"{name}: S"
        assert point(1) == V.flat(group, V.mul(group, want[1])), f"{name}: S'"
        spot = {0, len(chunks) - 1} | set(random.Random("pt_verify/spot/" + name).sample(range(len(chunks)), min(len(chunks), SPOT)))
        for t in sorted(spot if group == 1 else {len(chunks) - 1}):
            assert point(2 + t) == V.flat(group, V.mul(group, chunks[t])), f"{name}: chunk {t}"
        for t, c in enumerate(chunks):
            assert (point(2 + t) == [0] * per) == (c == 0), f"{name}: chunk {t}"


@pytest.mark.parametrize("group", (1, 2))
def test_cpu_loop_of_the_flags(native, group):
    kinds = V.bad_points(group)
    for name, (s, bad) in FLAGS[group].items():
        want = [kinds[bad[i]][1] if i in bad and bad[i] not in HOST_KINDS else 0 for i in range(len(s))]
        assert native[f"flags/{group}/{name}"] == want, name
    assert any(kinds[k][1] == V.SUBGROUP for k in kinds) == (group == 2)


def test_the_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "vimz_amd", "csrc", "g16_point_stage.hpp")).read()
    assert f"RLC_CHUNK = {V.RLC_CHUNK};" in src and f"PT_BLOCK = {V.PT_BLOCK};" in src
    assert f"PV_OFF_CURVE = {V.OFF_CURVE}, PV_IDENTITY = {V.IDENTITY}, PV_SUBGROUP = {V.SUBGROUP};" in src
    hdr = open(os.path.join(ROOT, "include", "vimz_hip.h")).read()
    for name, bit in (("COORD", V.COORD), ("OFF_CURVE", V.OFF_CURVE), ("IDENTITY", V.IDENTITY), ("SUBGROUP", V.SUBGROUP), ("FIRST", V.FIRST), ("RATIO_TAU_G1", V.RATIO_TAU_G1),
                      ("RATIO_ALPHA_G1", V.RATIO_ALPHA_G1), ("RATIO_BETA_G1", V.RATIO_BETA_G1), ("RATIO_TAU_G2", V.RATIO_TAU_G2), ("HALVES", V.HALVES), ("BETA", V.BETA)):
        assert f"#define VIMZ_POWERS_{name} 0x{bit:x}u" in hdr, name
    from vimz_amd import hip
    assert set(hip.POWERS_PROBLEMS) == {1 << k for k in range(11)} and hip.POWERS_ARRAYS == V.ARRAYS
