"""Packed curve points and packed decider keys on the GPU (vimz_points_pack / _unpack, vimz_decider_key_pack / _unpack; vimz_amd/csrc/g16_point_pack.hip and .hpp):
the kernels through the two point calls and the square root's hook, the two key calls on synthetic keys, the wrappers and commands, and once end to end on the light
decider of the hash step.

Every comparison is exact equality of words with tests/_point_pack_ref.py (plain Python integers over tests/_pairing.py); nothing is sampled.  Both groups and both
forms at n = 1, 2, 63, 64, 65, 129 and across a chunk boundary (VIMZ_PACK_CHUNK + 1 points tiled from a handful); points [s]G for s = 1, 2, r − 1 and random s, both
signs in every run from three points on; the identity first, last and everywhere.  Rejections with their index: x = q, x with no y (G1 x = 0, 4, 10, 12; G2 x = (0,0),
(0,2), (1,1)), INF with SIGN, INF with x != 0, a stray bit in a G2 word 3, and when packing a y off by one — the output untouched after each.  The GPU half is
tests/_point_pack_gpu.py, a process per part."""
import json
import os
import subprocess
import sys

import pytest

from tests import _key_contrib_ref as K
from tests import _point_pack_ref as ref
from tests._g16_kernels_gpu import hex_ints
from tests._pairing import Q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_part(tmp_path_factory, part, timeout):
    out = tmp_path_factory.mktemp("point_pack_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._point_pack_gpu", part, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
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


def _runs(group):
    runs = {f"{n}/none": ref.array(group, n) for n in ref.SIZES}
    runs.update({f"65/{ident}": ref.array(group, 65, ident) for ident in ("first", "last", "all")})
    runs["1/all"] = ref.array(group, 1, "all")
    return runs


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("group", [1, 2])
def test_points_pack_and_unpack_as_the_reference(kernels, group, mont):
    assert ref.SIZES == (1, 2, 63, 64, 65, 129)
    for name, data in _runs(group).items():
        key = f"g{group}/m{mont}/{name}"
        want = ref.run(group, True, data)[0]
        p, u = kernels["pack"][key], kernels["unpack"][key]
        assert (p["rc"], p["result"], p["first_bad"]) == (0, 0, 0) == (u["rc"], u["result"], u["first_bad"]), key
        assert bytes.fromhex(p["hex"]) == want, key                                  # the packed side is canonical in either form
        assert ref.from_form(bytes.fromhex(u["hex"]), mont) == data, key
        assert len(p["seconds"]) == 2 and p["seconds"][1] > 0
        if not name.endswith("all") and len(data) >= 3 * 64 * group:
            signs = {want[k] & 0x40 for k in range(32 * group - 1, len(want), 32 * group) if not want[k] & 0x80}
            assert signs == {0, 0x40}, key                                           # both signs are in the run
    inf = b"\0" * (32 * group - 1) + b"\x80"
    assert bytes.fromhex(kernels["pack"][f"g{group}/m{mont}/65/all"]["hex"]) == inf * 65
    assert bytes.fromhex(kernels["pack"][f"g{group}/m{mont}/65/first"]["hex"])[:32 * group] == inf
    assert bytes.fromhex(kernels["pack"][f"g{group}/m{mont}/65/last"]["hex"])[-32 * group:] == inf


@pytest.mark.parametrize("group", [1, 2])
def test_a_run_across_a_chunk_boundary(kernels, group):
    got = kernels[f"chunk_g{group}"]
    assert got["n"] == ref.chunk() + 1 and got["rc"] == [0, 0] and got["result"] == [0, 0]
    assert bytes.fromhex(got["small_packed"]) == ref.run(group, True, ref.array(group, 7, "first"))[0]
    assert got["packed_is_the_tiling"] and got["round_trip"]
    chunk = ref.chunk()
    assert got["spoiled"] == [[0, ref.COORD, chunk], [0, ref.FLAGS, chunk - 1], True]
    print(f"G{group}, {got['n']} points, seconds {{host, device with copies}}: pack {got['seconds'][0]}, unpack {got['seconds'][1]}")


@pytest.mark.parametrize("group", [1, 2])
def test_rejections_come_with_their_index_and_leave_the_output(kernels, group):
    asked = {"x_is_q", "inf_with_sign", "inf_with_x"} | ({f"no_y/{x}" for x in (0, 4, 10, 12)} if group == 1 else {"no_y/0_0", "no_y/0_2", "no_y/1_1", "stray_bit_62", "stray_bit_63"})
    assert asked <= set(ref.bad_packed(group)) and "y_off_by_one" in ref.bad_points(group)
    for mont in (0, 1):
        for name, (_data, finding) in ref.bad_packed(group).items():
            got = kernels["reject_unpack"][f"g{group}/m{mont}/{name}"]
            assert (got["rc"], got["result"], got["first_bad"], got["untouched"]) == (0, finding, got["at"], True), (name, got)
        for name, (_data, finding) in ref.bad_points(group).items():
            got = kernels["reject_pack"][f"g{group}/m{mont}/{name}"]
            assert (got["rc"], got["result"], got["first_bad"], got["untouched"]) == (0, finding, got["at"], True), (name, got)
    assert len(kernels["reject_unpack"]) == 2 * (len(ref.bad_packed(1)) + len(ref.bad_packed(2))) and len(kernels["reject_pack"]) == 2 * (len(ref.bad_points(1)) + len(ref.bad_points(2)))
    assert kernels[f"two_findings_g{group}"] == [0, ref.FLAGS, 9, True]


def test_the_device_root_over_fq2(kernels):
    got = kernels["fq2_sqrt"]
    vals = ref.sqrt_values()
    roots = hex_ints(got["roots"])
    assert got["rc"] == 0 and len(got["is_square"]) == len(vals)
    kinds = set()
    for k, a in enumerate(vals):
        want = ref.fq2_sqrt(a)
        assert got["is_square"][k] == (want is not None), a
        assert tuple(roots[2 * k:2 * k + 2]) == ref.fq2_sqrt_candidate(a), a          # the very root the algorithm forms, square or not
        if want is not None:
            assert ref.f2_sqr(want) == a
        kinds.add(("a1=0" if a[1] == 0 else "a0=0" if a[0] == 0 else "both", want is not None, want is not None and a[1] == 0 and want[0] == 0))
    # (a0, 0) with a0 a residue -> (t, 0); with a non-residue -> (0, t); (0, a1); squares and non-squares with both parts
    assert {("a1=0", True, False), ("a1=0", True, True), ("a0=0", True, False), ("both", True, False), ("both", False, False)} <= kinds
    assert tuple(roots[2 * vals.index((3, 0)):][:2])[0] == 0 and tuple(roots[2 * vals.index((4, 0)):][:2]) in ((2, 0), (Q - 2, 0))


def test_bad_arguments_of_the_point_calls(kernels):
    ba = kernels["bad_arguments"]
    assert len(ba) == 15 and all(rc == kernels["invalid"] for rc in ba.values()), ba
    ns = kernels["null_seconds"]
    assert (ns["rc"], ns["result"]) == (0, 0) and bytes.fromhex(ns["hex"]) == ref.run(1, True, ref.array(1, 5))[0]
    assert all((r["rc"], r["result"], r["first_bad"], r["untouched"]) == (0, 0, 0, True) for r in kernels["n_zero"])
    ip = kernels["pack_in_place"]
    assert (ip["rc"], ip["result"]) == (0, 0) and bytes.fromhex(ip["hex"]) == ref.run(2, True, ref.array(2, 9, "last"))[0]


# ---- the key calls ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "small_identity", "large", "large_identity"))
def test_keys_pack_and_unpack_as_the_reference(api, name):
    shape, identity = {"small": (K.SMALL, None), "small_identity": (K.SMALL, 3), "large": (K.LARGE, None), "large_identity": (K.LARGE, 3)}[name]
    key = K.synthetic_key(K.DELTA0, shape, identity)
    packed = ref.pack_key(key)[0]
    got = api["keys"][name]
    for way, want in (("pack", packed), ("unpack", key), ("pack_in_place", packed), ("unpack_in_place", key)):
        g = got[way]
        assert (g["rc"], g["result"], g["first_bad"]) == (len(want), 0, [0, 0]), (name, way, g["message"])
        assert bytes.fromhex(g["hex"]) == want, (name, way)
    assert len(packed) == ref.packed_size(len(key)) == 88 + (len(key) - 88) // 2


def test_a_short_cap_returns_the_size_and_writes_nothing(api):
    sc = api["short_cap"]
    assert sc["sizes"] == [sc["pack"]["rc"], sc["unpack"]["rc"]] == [sc["pack_no_out"], sc["unpack_no_out"]]
    assert sc["pack"]["untouched"] and sc["unpack"]["untouched"]


def test_refused_blobs_and_bad_arguments_of_the_key_calls(api):
    assert len(api["bad_arguments"]) == 8 and all(rc == api["invalid"] for rc in api["bad_arguments"].values()), api["bad_arguments"]
    want = {"pack_truncated": "vimz_decider_key_pack: wrong length", "pack_oversized": "vimz_decider_key_pack: wrong length", "pack_a_packed_key": "vimz_decider_key_pack: not a decider key",
            "unpack_truncated": "vimz_decider_key_unpack: wrong length", "unpack_oversized": "vimz_decider_key_unpack: wrong length",
            "unpack_a_plain_key": "vimz_decider_key_unpack: not a packed decider key", "unpack_one_byte": "vimz_decider_key_unpack: not a packed decider key",
            "unpack_wrong_magic": "vimz_decider_key_unpack: not a packed decider key"}
    assert {k: (r["rc"], r["message"], r["untouched"]) for k, r in api["refused"].items()} == {k: (api["invalid"], m, True) for k, m in want.items()}


@pytest.mark.parametrize("name", sorted(ref.key_point_words(K.LARGE)))
def test_a_tampered_point_in_each_part_of_a_key(api, name):
    _group, off, poff = ref.key_point_words(K.LARGE)[name]
    key = K.synthetic_key(K.DELTA0, K.LARGE)
    got = api["tampered"][name]
    assert (got["pack"]["rc"], got["pack"]["result"], got["pack"]["first_bad"], got["pack"]["untouched"]) == (ref.packed_size(len(key)), ref.OFF_CURVE, [off, ref.OFF_CURVE], True)
    assert (got["unpack"]["rc"], got["unpack"]["result"], got["unpack"]["first_bad"], got["unpack"]["untouched"]) == (len(key), ref.COORD, [poff, ref.COORD], True)


def test_a_tampered_point_on_a_chunk_boundary_of_a_key(api):
    bd = api["boundary"]
    assert bd["n_g1"] > bd["chunk"] == ref.chunk() and bd["clean"] == [bd["bytes"][1], 0, bd["bytes"][0], 0] and bd["round_trip"]
    assert bd["bytes"][1] == ref.packed_size(bd["bytes"][0])
    for label in ("last_of_chunk_0", "first_of_chunk_1", "last_g1"):
        rc, result, first, untouched, word = bd["pack"][label]
        assert (rc, result, first, untouched) == (bd["bytes"][1], ref.OFF_CURVE, [word, ref.OFF_CURVE], True), label
        rc, result, first, untouched, word = bd["unpack"][label]
        assert (rc, result, first, untouched) == (bd["bytes"][0], ref.COORD, [word, ref.COORD], True), label
    assert bd["pack"]["first_of_chunk_1"][4] == ref.KEY_IC + 8 * ref.chunk() and bd["unpack"]["first_of_chunk_1"][4] == ref.PKEY_IC + 4 * ref.chunk()


def test_python_wrappers(api):
    py = api["python"]
    pts = ref.array(2, 9, "first")
    assert bytes.fromhex(py["pack_points"]) == ref.run(2, True, pts)[0] and py["shape"] == [9, 8] and bytes.fromhex(py["unpack_points"]) == pts
    assert len(py["seconds"]) == 2 and py["empty"] == [[0, 4], [0, 8]]
    key = K.synthetic_key(K.DELTA0, K.LARGE)
    assert bytes.fromhex(py["pack_key"]) == ref.pack_key(key)[0] and bytes.fromhex(py["unpack_key"]) == key and py["key_is_packed"] == [True, False, False]
    assert len(py["problems"]) == 2
    origin, final, records = K.chain(K.LARGE, 1)
    cp = py["contribute_packed"]
    assert cp["is_packed"] and bytes.fromhex(cp["key"]) == ref.pack_key(final)[0] and bytes.fromhex(cp["record"]) == records      # the form it was given
    assert py["verify_mixed"] == [[0, [0, 0]]] * 4
    rf = py["refusals"]
    assert all(code == api["invalid"] for code, _m in rf.values())
    assert "point 4" in rf["unpack_points"][1] and "FLAGS" in rf["unpack_points"][1] and "OFF_CURVE" in rf["pack_key"][1] and f"word {ref.KEY_IC}" in rf["pack_key"][1]
    assert "not a packed decider key" in rf["unpack_key_not_packed"][1]


def test_strings_pack_and_unpack(api):
    pw = api["powers"]
    n2 = 8
    points_bytes = 64 * (2 * n2 - 1) + 128 * n2 + 64 * n2 + 64 * n2 + 128
    assert pw["magic"] == "VPOTPK01" and pw["head"] == [3, 0, 0, 0, 3, 0, 0, 0] and pw["bytes"][0] == 16 + points_bytes // 2
    assert pw["same_file"] and pw["verify"] == [0, [0, 0]]
    # the packed side is canonical: tau_g1[1]'s packed x is the file's Montgomery x brought back
    packed_x = int.from_bytes(bytes.fromhex(pw["tau_g1_1"][0]), "little") & ((1 << 254) - 1)
    assert packed_x == int.from_bytes(bytes.fromhex(pw["tau_g1_1"][1])[:32], "little") * pow(1 << 256, -1, Q) % Q
    assert pw["refusals"]["truncated"].startswith("ValueError") and pw["refusals"]["magic"].startswith("ValueError")
    assert pw["refusals"]["bad_point"].startswith(f"VimzError {api['invalid']}") and "point 0" in pw["refusals"]["bad_point"]


def test_every_new_command_with_its_exit_status(api):
    cli = api["cli"]
    for name in ("pack_key", "unpack_key", "contribute_packed", "verify_plain_origin", "verify_packed_origin", "pack_powers", "unpack_powers"):
        assert cli[name]["rc"] == 0, (name, cli[name])
    assert "accepted" in cli["verify_plain_origin"]["stdout"] and "accepted" in cli["verify_packed_origin"]["stdout"]
    assert all(cli[f"usage_{name}"]["rc"] == 2 for name in ("pack_key", "unpack_key", "pack_powers", "unpack_powers"))
    assert cli["files"] == {"packed_key": True, "back_key": True, "one_key_is_packed": True, "packed_powers": True, "back_ptau": True}
    assert cli["unpack_a_plain_key"] == f"VimzError {api['invalid']}"


# ---- end to end, once: the light decider of the hash step ------------------------------------------------------------------------------------------------
def test_a_packed_key_is_half_the_bytes_and_unpacks_to_save_key(decider):
    info = decider["info"]
    assert info["domain"] == 1 << 18
    m, n_pub, n = info["wires"], info["public_inputs"], info["domain"]
    L = ref.runs(m, n_pub, n)
    assert decider["sizes"] == {"plain": 8 * L["words"], "packed": 8 * L["pwords"]}      # 8·(99 + 8·n_g1 + 16·m) and 8·(55 + 4·n_g1 + 8·m) bytes
    assert decider["sizes"]["packed"] == 88 + (decider["sizes"]["plain"] - 88) // 2
    assert decider["is_packed"] == [True, False] and decider["unpack_is_save_key"] and decider["pack_of_unpack"]
    print("light hash decider's key:", decider["sizes"], "wall seconds:", decider["wall_seconds"])


def test_a_proof_under_the_loaded_packed_key(decider):
    pr = decider["proof"]
    assert pr["verify"] == 0 and pr["verify_wrong_steps"] != 0 and pr["light"] is True and pr["info"] == decider["info"]


def test_contributions_with_either_form_on_either_side(decider):
    c = decider["contribute"]
    assert c["is_packed"] == [True, False] and c["same_key"] and c["same_record"] and c["bytes"] == [decider["sizes"]["packed"], decider["sizes"]["plain"]]
    assert decider["chains"] == {k: [0, [0, 0]] for k in ("plain_plain", "plain_packed", "packed_plain", "packed_packed")}
    assert decider["chain_against_itself"][0] == K.LAST
