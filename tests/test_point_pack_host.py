"""The per-thread functions of k_points_pack and k_points_unpack and the host's parser of a packed key (vimz_amd/csrc/g16_point_pack.hpp: pt_pack, pt_unpack, fq_sqrt,
fq2_sqrt, packed_key_layout) without a GPU.

tests/native/point_pack_check.cpp, built with g++ -fsanitize=address,undefined and run directly, loops pt_pack and pt_unpack over every thread index at n = 1, 2, 63,
64 and 65 from heap blocks of exact size, for G1 and G2 and both forms — checking after every thread that it wrote its own slot and its own flag and nothing else —,
and runs the parser over good, truncated, oversized, one-byte and wrong-magic blobs.  Here its words against tests/_point_pack_ref.py."""
import os
import subprocess

import pytest

from tests import _key_contrib_ref as kref
from tests import _point_pack_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 63, 64, 65)


def arrays():
    """name -> (group, mont, canonical point bytes): per group, form and size a run of points; the identity first, last and everywhere; the points that must not
    pack between good ones"""
    cases = {}
    for group in (1, 2):
        for mont in (0, 1):
            for n in SIZES:
                cases[f"g{group}/m{mont}/{n}/points"] = (group, mont, ref.array(group, n))
            for identity in ("first", "last", "all"):
                cases[f"g{group}/m{mont}/65/identity_{identity}"] = (group, mont, ref.array(group, 65, identity))
            cases[f"g{group}/m{mont}/1/identity"] = (group, mont, ref.array(group, 1, "all"))
            good = ref.point_bytes(group, 7)
            cases[f"g{group}/m{mont}/bad"] = (group, mont, good + b"".join(data + good for data, _ in ref.bad_points(group).values()))
    return cases


def packed_arrays():
    """name -> (group, mont, packed bytes): the arrays above packed by the reference, and the encodings that must not unpack between good ones"""
    cases = {}
    for name, (group, mont, data) in arrays().items():
        if not name.endswith("/bad"):
            cases[name] = (group, mont, ref.run(group, True, data)[0])
    for group in (1, 2):
        good = ref.pack_point_bytes(group, ref.point_bytes(group, 7))[0]
        for mont in (0, 1):
            cases[f"g{group}/m{mont}/bad"] = (group, mont, good + b"".join(data + good for data, _ in ref.bad_packed(group).values()))
    return cases


def key_blobs():
    packed = ref.pack_key(kref.synthetic_key(kref.DELTA0, kref.SMALL))[0]
    large = ref.pack_key(kref.synthetic_key(kref.DELTA0, kref.LARGE, 3))[0]
    return {"small": packed, "large": large, "truncated": packed[:-8], "oversized": packed + bytes(8), "one_byte": packed[:1], "empty": b"", "odd_length": packed[:-3],
            "head_only": packed[:8 * ref.PKEY_IC], "short": packed[:64], "wrong_magic": kref.put(packed, 0, b"VG16KEY2"), "a_plain_key": kref.synthetic_key(kref.DELTA0, kref.SMALL),
            "mode_2": kref.put(packed, 6, (2).to_bytes(8, "little")), "n_zero": kref.put(packed, 4, bytes(8)), "m_huge": kref.put(packed, 1, (1 << 31).to_bytes(8, "little")),
            "m_lies": kref.put(packed, 1, (7).to_bytes(8, "little")), "n_pub_is_m": kref.put(packed, 2, (6).to_bytes(8, "little"))}


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("point_pack")
    exe, spec = d / "point_pack_check", d / "cases.txt"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "point_pack_check.cpp")])
    lines = [f"PACK pack/{name} {g} {mont} {len(data) // (64 * g)} {ref.to_form(data, mont).hex()}" for name, (g, mont, data) in arrays().items()]
    lines += [f"UNPACK unpack/{name} {g} {mont} {len(data) // (32 * g)} {data.hex()}" for name, (g, mont, data) in packed_arrays().items()]
    lines += [f"PARSE parse/{name} {blob.hex() or '-'}" for name, blob in key_blobs().items()]
    spec.write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(spec)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def _slots(tokens):
    return [(bytes.fromhex(t.split(":")[1]), int(t.split(":")[0])) for t in tokens]


def test_every_case_is_reported(native):
    assert set(native) == {f"pack/{n}" for n in arrays()} | {f"unpack/{n}" for n in packed_arrays()} | {f"parse/{n}" for n in key_blobs()}


def test_cpu_loop_of_packing(native):
    for name, (group, _mont, data) in arrays().items():
        assert _slots(native[f"pack/{name}"]) == ref.per_point(group, True, data), name
    for group in (1, 2):
        flags = [f for _, f in _slots(native[f"pack/g{group}/m1/bad"])]
        assert flags == [0] + [x for _, f in ref.bad_points(group).values() for x in (f, 0)]
        assert ref.COORD in flags and ref.OFF_CURVE in flags


def test_cpu_loop_of_unpacking(native):
    for name, (group, mont, data) in packed_arrays().items():
        got = [(ref.from_form(slot, mont), f) for slot, f in _slots(native[f"unpack/{name}"])]
        assert got == ref.per_point(group, False, data), name
    for group in (1, 2):
        flags = [f for _, f in _slots(native[f"unpack/g{group}/m0/bad"])]
        assert flags == [0] + [x for _, f in ref.bad_packed(group).values() for x in (f, 0)]
        assert {ref.COORD, ref.FLAGS, ref.OFF_CURVE} <= set(flags)
    # the round trip, on the native words alone
    for name, (group, mont, data) in arrays().items():
        if not name.endswith("/bad"):
            assert b"".join(ref.from_form(slot, mont) for slot, _ in _slots(native[f"unpack/{name}"])) == data, name


def test_the_packed_key_parser(native):
    for name, blob in key_blobs().items():
        try:
            L = ref.packed_layout(blob)
            want = ["ok", str(L["n_g1"]), str(L["n_g2"]), str(L["words"]), str(L["pwords"])]
        except ValueError as e:
            want = ["err"] + str(e).split()
        assert native[f"parse/{name}"] == want, name
    assert native["parse/small"][0] == native["parse/large"][0] == "ok"
    assert [native[f"parse/{n}"][0] for n in key_blobs() if n not in ("small", "large")] == ["err"] * (len(key_blobs()) - 2)
    assert native["parse/truncated"][1:] == native["parse/oversized"][1:] == native["parse/m_lies"][1:] == ["wrong", "length"]


def test_the_constants_are_the_kernels():
    hpp = open(os.path.join(ROOT, "vimz_amd", "csrc", "g16_point_pack.hpp")).read()
    assert f"PACKED_KEY_MAGIC = 0x{ref.PACKED_KEY_MAGIC:x}ull" in hpp
    assert f"PKEY_KZG = {ref.PKEY_KZG}, PKEY_ALPHA1 = {ref.PKEY_ALPHA1}, PKEY_BETA2 = {ref.PKEY_BETA2}, PKEY_IC = {ref.PKEY_IC};" in hpp
    assert f"KEY_KZG = {ref.KEY_KZG}, KEY_ALPHA1 = {ref.KEY_ALPHA1}, KEY_BETA2 = {ref.KEY_BETA2};" in hpp
    assert ref.chunk() == 1 << 20
    h = open(os.path.join(ROOT, "include", "vimz_hip.h")).read()
    assert f"VIMZ_PACK_COORD 0x{ref.COORD:x}u" in h and f"VIMZ_PACK_FLAGS 0x{ref.FLAGS:x}u" in h and f"VIMZ_PACK_OFF_CURVE 0x{ref.OFF_CURVE:x}u" in h
