"""The per-thread functions of k_power_vec and k_scale_points_by and the host code of a contribution to a powers-of-tau string (vimz_amd/csrc/g16_point_stage.hpp:
pt_power, pt_scale_by; g16_powers_contrib.hpp: make_powers_record, powers_record_knowledge, powers_records_layout) without a GPU.

tests/native/powers_contrib_check.cpp, built with g++ -fsanitize=address,undefined and run directly, loops pt_power and pt_scale_by over every thread index at n = 1,
2, 7, 8 and 9 from heap blocks of exact size, in place and out of place, for G1 and G2 — checking after every thread that it wrote its own slot and no other —, makes
and checks records (a zero nonce among them) and parses good, truncated, oversized and wrong-magic record blocks.  Here its words against tests/_powers_contrib_ref.py."""
import os
import subprocess

import pytest

from tests import _powers_contrib_ref as K
from tests import _powers_verify_ref as V
from tests._pairing import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 7, 8, 9)
RECORDS = {"first": (K.triple(K.chain_scalars(1)[0]), K.SECRET_SETS[0], K.NONCE_SETS[0]), "second": (K.triple(K.chain_scalars(1)[1]), K.SECRET_SETS[1], K.NONCE_SETS[1]),
           "nonce_zero": ((5, 6, 7), (7, 8, 9), (0, 3, 0)), "small": ((1, 1, 1), (2, 1, R - 1), (1, 2, 3))}


def scale_inputs():
    """name -> (group, n, in_place, w, c, scalars): per group and size the random walk out of place and in place, w = r − 1, w = c = 1 and c = 0"""
    cases = {}
    for group in (1, 2):
        for n in SIZES:
            s = K.scale_inputs(n)
            if n == 9:
                s[1] = 1
            cases[f"g{group}/{n}/random"] = (group, n, 0, K.W_RANDOM, K.C_RANDOM, s)
            cases[f"g{group}/{n}/in_place"] = (group, n, 1, K.W_RANDOM, K.C_RANDOM, s)
            cases[f"g{group}/{n}/w_r_minus_1"] = (group, n, 1, R - 1, 1, s)
            cases[f"g{group}/{n}/ones"] = (group, n, 0, 1, 1, s)
            cases[f"g{group}/{n}/c_zero"] = (group, n, 0, 2, 0, s)
    return cases


def record_blocks():
    recs = K.chain_records(3)
    return {"none": b"", "three": recs, "truncated": recs[:-8], "one_byte": recs[:1], "oversized": recs + bytes(8), "wrong_magic_first": K.put(recs, 0, b"VPOTCTR2"),
            "wrong_magic_last": K.put(recs, 2 * K.RECORD_WORDS, b"VG16CTR1"), "a_key_record": bytes(296)}


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("powers_contrib")
    exe, spec = d / "powers_contrib_check", d / "cases.txt"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "powers_contrib_check.cpp")])
    lines = [f"POWER power/{n}/{name} {n} {w:x}" for n in SIZES for name, w in K.POWER_WS.items()]
    lines += [f"SCALE scale/{name} {g} {n} {ip} {w:x} {c:x} " + " ".join(f"{x:x}" for x in s) for name, (g, n, ip, w, c, s) in scale_inputs().items()]
    lines += [f"RECORD record/{name} " + " ".join(f"{x:x}" for x in b + s + k) for name, (b, s, k) in RECORDS.items()]
    lines += [f"PARSE parse/{name} {blob.hex() or '-'}" for name, blob in record_blocks().items()]
    spec.write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(spec)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_every_case_is_reported(native):
    assert set(native) == ({f"power/{n}/{w}" for n in SIZES for w in K.POWER_WS} | {f"scale/{n}" for n in scale_inputs()} | {f"record/{n}" for n in RECORDS}
                           | {f"parse/{n}" for n in record_blocks()})


def test_cpu_loop_of_the_power_vector(native):
    for n in SIZES:
        for name, w in K.POWER_WS.items():
            assert [int(x, 16) for x in native[f"power/{n}/{name}"]] == [pow(w, i, R) for i in range(n)], (n, name)


def test_cpu_loop_of_the_scaling(native):
    for name, (group, n, _ip, w, c, s) in scale_inputs().items():
        want = [x for e in K.scale_expected(s, w, c) for x in V.flat(group, V.mul(group, e))]
        assert [int(x, 16) for x in native[f"scale/{name}"]] == want, name
    assert all(int(x, 16) == 0 for x in native["scale/g2/9/c_zero"])            # every output the identity
    assert native["scale/g1/8/ones"][2:4] != ["0" * 64] * 2                      # ... and not because everything is


def test_the_record_maker_and_checker(native):
    for name, (b, s, k) in RECORDS.items():
        rec = K.make_record(K.scalar_points(b), s, k)
        assert len(rec) == K.RECORD_BYTES
        assert native[f"record/{name}"] == [rec.hex(), "0", "1", "2", "4", "7"], name
        assert K.knowledge_failed(K.scalar_points(b), rec) == 0
    assert K.chain_records(3)[:2 * K.RECORD_BYTES].hex() == native["record/first"][0] + native["record/second"][0]
    assert K.record_points(bytes.fromhex(native["record/nonce_zero"][0]))[1][0] == (0, 0)      # T of a zero nonce is the identity


def test_the_record_parser(native):
    want = {"none": ["ok", "0"], "three": ["ok", "3"], "truncated": ["err", "0"], "one_byte": ["err", "0"], "oversized": ["err", "0"], "wrong_magic_first": ["err", "0"],
            "wrong_magic_last": ["err", "2"], "a_key_record": ["err", "0"]}
    for name, blob in record_blocks().items():
        assert native[f"parse/{name}"][:2] == want[name], name
        try:
            K.split_records(blob)
            assert want[name][0] == "ok", name
        except ValueError:
            assert want[name][0] == "err", name


def test_the_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "vimz_amd", "csrc", "g16_point_stage.hpp")).read()
    assert f"PT_BLOCK = {K.PT_BLOCK};" in src
    hpp = open(os.path.join(ROOT, "vimz_amd", "csrc", "g16_powers_contrib.hpp")).read()
    assert f"RECORD_WORDS = {K.RECORD_WORDS}, REC_A = {K.REC_A}, REC_T = {K.REC_T}, REC_Z = {K.REC_Z};" in hpp and K.TAG.decode() in hpp
    assert f"0x{K.RECORD_MAGIC:x}ull" in hpp
