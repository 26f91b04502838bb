"""The per-thread function of k_ratio_rlc and the host code of a key contribution (vimz_amd/csrc/g16_point_stage.hpp: pt_ratio_chunk; g16_key_contrib.hpp: key_layout,
make_record, record_knowledge) without a GPU.

tests/native/key_contrib_check.cpp, built with g++ -fsanitize=address,undefined and run directly, loops pt_ratio_chunk over every thread index of both grid rows at
n = 1, 7, 8, 9 and 19 — checking after every thread that it wrote its own slot and no other —, reduces the chunk sums through the two-column plan, parses good,
truncated, oversized and lying blobs from heap blocks of their exact size, and makes and checks records.  Here its words against tests/_key_contrib_ref.py."""
import os
import subprocess

import pytest

from tests import _key_contrib_ref as K
from tests._pairing import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 7, 8, 9, 19)


def ratio_inputs():
    """name -> (before, after, rho) on scalars: the reference's cases at the sizes a CPU loop affords, and per size one whose arrays hold an identity each at
    DIFFERENT indices (the kernel sums; the host judges)"""
    cases = {name: c for name, c in K.ratio_cases().items() if int(name.split("/")[0]) in SIZES + (2,)}
    for n in SIZES:
        rho = K.fixed_rho(n, "native")
        before, after = [K.BASE_D * (k + 1) % R for k in range(n)], [K.BASE_D * (3 * k + 2) % R for k in range(n)]
        before[0], after[-1] = 0, 0
        cases[f"{n}/identities_apart"] = (before, after, rho)
    return cases


def blobs():
    key = K.synthetic_key(K.DELTA0)
    out = {name: blob for name, (blob, _msg) in K.refused_keys().items() if name in ("wrong_magic", "truncated", "oversized", "short", "odd_length")}
    out.update({"good": key, "large": K.synthetic_key(K.DELTA0, K.LARGE), "empty": b"", "header_only": key[:56], "just_below_ic": key[:8 * K.KEY_IC - 8],
                "m_is_2_to_40": K.put(key, 1, (1 << 40).to_bytes(8, "little")), "n_pub_is_m": K.put(key, 2, (6).to_bytes(8, "little")), "n_is_0": K.put(key, 4, bytes(8)),
                "mode_2": K.put(key, 6, (2).to_bytes(8, "little")), "n_is_larger": K.put(key, 4, (5).to_bytes(8, "little"))})
    return out


RECORDS = {"first": (K.DELTA0, K.DELTAS[0], K.NONCES[0]), "second": (K.DELTA0 * K.DELTAS[0] % R, K.DELTAS[1], K.NONCES[1]), "nonce_zero": (5, 7, 0), "small": (1, 2, 1)}


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("key_contrib")
    exe, spec = d / "key_contrib_check", d / "cases.txt"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "key_contrib_check.cpp")])
    head = K.synthetic_key(K.DELTA0)[:88].hex()
    lines = [f"RATIO ratio/{name} {len(r)} " + " ".join(f"{x:x}" for x in b + a + r) for name, (b, a, r) in ratio_inputs().items()]
    lines += [f"PARSE parse/{name} {blob.hex() or '-'}" for name, blob in blobs().items()]
    lines += [f"RECORD record/{name} {head} {s:x} {d:x} {k:x}" for name, (s, d, k) in RECORDS.items()]
    spec.write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(spec)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_every_case_is_reported(native):
    assert set(native) == {f"ratio/{n}" for n in ratio_inputs()} | {f"parse/{n}" for n in blobs()} | {f"record/{n}" for n in RECORDS}
    assert {len(r) for _b, _a, r in ratio_inputs().values()} == set(SIZES) | {2}


def test_cpu_loop_of_the_combination(native):
    point = lambda s: list(K.bp.g1_mul(K.bp.G1, s) or (0, 0))      # noqa: E731
    for name, (before, after, rho) in ratio_inputs().items():
        got = [int(w, 16) for w in native[f"ratio/{name}"]]
        cb, ca = K.ratio_chunk_scalars(before, rho), K.ratio_chunk_scalars(after, rho)
        assert len(got) == 2 * (2 + 2 * len(cb)), name
        s, s1 = K.ratio_scalars(before, after, rho)
        assert got[0:2] == point(s) and got[2:4] == point(s1), name
        for t, c in enumerate(cb + ca):                             # row 0's slots, then row 1's
            assert got[4 + 2 * t:6 + 2 * t] == point(c), f"{name}: slot {t}"


def test_the_parser(native):
    for name, blob in blobs().items():
        try:
            L = K.layout(blob)
            want = ["ok", str(L["words"]), str(L["off_lh"]), str(L["n_lh"])]
        except ValueError as e:
            want = ["err"] + str(e).split()
        assert native[f"parse/{name}"] == want, name
    assert native["parse/good"][0] == "ok" == native["parse/large"][0] and sum(native[f"parse/{n}"][0] == "err" for n in blobs()) == len(blobs()) - 2


def test_the_record_maker_and_checker(native):
    head = K.synthetic_key(K.DELTA0)[:88]
    for name, (s, d, k) in RECORDS.items():
        rec, _a1, _a2 = K.make_record(head, K.bp.g1_mul(K.bp.G1, s), K.bp.g2_mul(K.bp.G2, s), d, k)
        assert native[f"record/{name}"] == [rec.hex(), "1", "0", "0"], name
    assert K.chain(K.SMALL, 3)[2][:2 * K.RECORD_BYTES].hex() == native["record/first"][0] + native["record/second"][0]


def test_the_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "vimz_amd", "csrc", "g16_point_stage.hpp")).read()
    assert f"RLC_CHUNK = {K.RLC_CHUNK};" in src and f"PT_BLOCK = {K.PT_BLOCK};" in src
