"""Many compressed proofs in one call, on the GPU (vimz_ivc_verify_compressed_batch, vimz_cf_verify_compressed_batch; vimz_amd/csrc/spartan_batch.hpp): the two
new kernels through their hooks word for word against tests/_spartan_batch_ref.py (tied to the protocol on the CPU by tests/test_spartan_batch_ref_host.py), the
chunk and fallback logic on a caller's instances, and both entry points end to end on `hash` at HD.  Equality is of words; there is no tolerance anywhere.

k_svec_accum: rounds 1, 2, log2(block) − 1, log2(block), log2(block) + 1, h − 1, h, h + 1 and 13 on both fields, groups of 1, the group size and the group size + 1,
shifted and unshifted openings mixed (slot 0 of a shifted opening lands on the key's last point), masks at n_pub 1 and 7 with n_w = N and N/2 + 1, a challenge 0
and a challenge r − 1; rounds 19 with three openings by digest.  k_mat_eval: the instance shapes of tests/_spartan_ref.py (their dense ones carry long and medium
rows and repeated triplets), a shape with an empty row, a medium row, a long row and a repeated triplet, the same with an empty matrix, groups of 1, G and G + 1.
The GPU half is tests/_spartan_batch_gpu.py, a process a part."""
import json
import os
import subprocess
import sys

import pytest

from tests import _oracle
from tests import _spartan_batch_gpu as G
from tests import _spartan_batch_ref as B
from tests import _spartan_pub_ref as P
from tests import _spartan_ref as S
from tests._oracle import CURVE_SCALAR
from vimz_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_part(tmp_path_factory, part, timeout):
    out = tmp_path_factory.mktemp("spartan_batch_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._spartan_batch_gpu", part, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def svec(tmp_path_factory):
    return run_part(tmp_path_factory, "svec", 600)


@pytest.fixture(scope="module")
def mat(tmp_path_factory):
    return run_part(tmp_path_factory, "mat", 600)


@pytest.fixture(scope="module")
def instance(tmp_path_factory):
    return run_part(tmp_path_factory, "instance", 600)


@pytest.fixture(scope="module")
def ivc(tmp_path_factory):
    return run_part(tmp_path_factory, "ivc", 900)["ivc"]


@pytest.fixture(scope="module")
def cf(tmp_path_factory):
    return run_part(tmp_path_factory, "cf", 900)["cf"]


@pytest.fixture(scope="module")
def orc():
    return _oracle.load()


# ---- k_svec_accum ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_tests_know_the_kernels_constants(svec):
    assert (svec["group"], svec["split"]) == (B.GROUP, B.SPLIT_H)
    assert sorted(svec["case"]) == sorted(B.svec_case_names())
    seen = set()
    for name in B.svec_case_names():
        for op in B.svec_case(name)["ops"]:
            if op["n_w"]:
                N = 1 << int(name.split("/")[1])
                seen.add((op["n_pub"], "N" if op["n_w"] == N else "N/2+1"))
    assert seen >= {(1, "N"), (1, "N/2+1"), (7, "N"), (7, "N/2+1")}


@pytest.mark.parametrize("name", B.svec_case_names())
def test_svec_accum_word_for_word(svec, name):
    case = B.svec_case(name)
    acc, dots = B.svec_expected(case)
    got = svec["case"][name]
    raw = bytes.fromhex(got["acc"])
    got_acc = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    assert len(got_acc) == len(acc)
    bad = [j for j, (a, b) in enumerate(zip(got_acc, acc)) if a != b]
    assert not bad, f"{name}: accumulator slots {bad[:8]} differ"
    assert [int(x) for x in got["dots"]] == dots
    # slot 0 of a shifted opening is the key's LAST point: alone in a group, its s[0] = 1 lands there
    if name.endswith("/1") and case["ops"][0]["shifted"]:
        assert got_acc[-1] == case["ops"][0]["coef"]


def test_svec_accum_at_the_workload_s_grid_size(svec):
    digests, dots = B.svec_big_expected(B.svec_big_case())
    assert svec["big"]["digests"] == digests
    assert [int(x) for x in svec["big"]["dots"]] == dots


# ---- k_mat_eval -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.mat_shape_cases())
def test_mat_eval_on_the_instance_shapes(mat, name):
    case = S.instance_case(name)
    p = S.FIELD[CURVE_SCALAR[case["cid"]]]
    for n in B.MAT_GROUPS:
        want = [B.mat_eval(case, rx, ry, w, p) for rx, ry, w in B.mat_points(case, n, name)]
        assert [int(x) for x in mat["shape"][name][str(n)]] == want, (name, n)


@pytest.mark.parametrize("key", ["0/mixed", "0/empty", "1/mixed", "1/empty"])
def test_mat_eval_on_rows_of_every_class(mat, key):
    cid, kind = key.split("/")
    case = B.mat_special_case(int(cid), kind)
    rows = {}
    for r, c, v in case["A"]:
        rows[r] = rows.get(r, 0) + 1
    assert 3 not in rows and 7 <= rows[4] <= 32 < rows[5] and (kind == "mixed") == bool(case["B"])
    p = S.FIELD[CURVE_SCALAR[case["cid"]]]
    for n in B.MAT_GROUPS:
        want = [B.mat_eval(case, rx, ry, w, p) for rx, ry, w in B.mat_points(case, n, key)]
        assert [int(x) for x in mat["special"][key][str(n)]] == want, (key, n)


# ---- the chunk logic on a caller's instances --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", (0, 1))
def test_instances_honest_and_with_a_wrong_final_scalar(instance, cid):
    r = instance[str(cid)]
    assert (r["single_good"], r["single_bumpW"], r["single_bumpE"]) == (1, 0, 0)
    assert r["honest"] == {"0": [1] * 5, "1": [1] * 5, "2": [1] * 5} and r["empty"] == []
    for ch in ("0", "1", "2"):
        m = r["mixed"][ch]
        assert m["results"] == [1, 0, 1, 1, 0], (cid, ch)          # the bad members are refused alone, their chunk-mates keep their word
        assert m["seconds"][5] > 0                               # the fallback's share
        assert all(x >= 0 for x in m["seconds"])


@pytest.mark.parametrize("cid", (0, 1))
def test_public_elements_and_strict_instances(instance, cid):
    r = instance[str(cid)]
    pub = r["public"]
    assert pub["single"][0] == 1 and not any(pub["single"][1:])
    assert pub["batch"] == {"0": pub["single"], "2": pub["single"]}
    sb = r["strict_beside"]
    assert sb["single"] == [1, 1, 1, 0, 0]
    assert sb["batch"] == {"0": sb["single"], "2": sb["single"]}


@pytest.mark.parametrize("cid", (0, 1))
def test_multipliers(instance, orc, cid):
    r = instance[str(cid)]
    # all multipliers one: the accumulators are the reference's
    strict = P.case(G.INSTANCE_SHAPES[cid] + "/strict")
    ps = S.FIELD[CURVE_SCALAR[cid]]
    rng = S._rng("batch-instance", cid)
    c = dict(strict)
    c["Z"] = [rng.randrange(1, ps) for _ in range(strict["n_w"])]
    az, bz, cz = S.products(c)
    c["E"] = [(x * y - c["Z"][0] * w) % ps for x, y, w in zip(az, bz, cz)]
    _, blob = P.prove(orc, c)
    d = B.deferred_bytes(c, blob, P.LABEL)
    big = 1 << (max(c["n_c"], c["n_w"]) - 1).bit_length()
    holds, acc = B.batch_holds(orc, cid, d["openings"] * 3, [1] * 6, big)
    assert holds and r["ones"]["results"] == [1, 1, 1]
    assert [int(x) for x in r["ones"]["acc"]] == acc
    assert r["zero_multiplier"] == instance["invalid"] == _lib.ERR_INVALID
    # the production entry refuses the wrong member whatever the OS draws
    assert r["production_bump"] == [[1, 0]] * 3


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------------
def _family(r, last_bit, middle_bit):
    single = r["single"]
    by = dict(zip(r["what"], single))
    assert by["chain5"] == by["chain3"] == by["merged6"] == by["merged4"] == 0
    assert by["chain5 steps+1"] & 4096 and by["merged4 steps-1"] & 4096 and by["chain5 other z0"] & (4096 | 1) == (4096 | 1)
    assert by["chain5 last argument"] == last_bit and by["chain5 middle argument"] == middle_bit and by["chain3 first argument"] == 4
    assert by["merged6 last argument"] == 8 and by["merged6 first argument"] == 4
    assert by["chain3 truncated"] == by["other family"] == by["merged6 truncated"] == 8192
    assert by["chain5 instance"] != 0 and by["chain5 sum-check message"] & 4
    # the second hash, with the blob well-formed: bit 1, and not the malformed bit
    assert by["chain5 second hash"] & 2 and not by["chain5 second hash"] & 8192
    assert by["merged6 second hash"] & 2 and not by["merged6 second hash"] & 8192
    seen = 0
    for w in single:
        seen |= w
    assert seen & (1 | 2 | 4 | 8 | 16 | 4096 | 8192) == (1 | 2 | 4 | 8 | 16 | 4096 | 8192)          # every bit the single verifiers can set
    # good and bad members alternate: every chunk of two mixes them
    assert [w == 0 for w in single[:8]] == [True, False] * 4
    for ch in ("0", "1", "2"):
        assert r["batch"][ch] == single, f"chunk {ch}"
    assert r["folding"] == single and r["empty"] == []
    assert r["honest"]["words"] == [0, 0, 0, 0] and r["honest"]["seconds"]["fallback_s"] < 1e-4 and r["honest"]["seconds"]["msm_s"] > 0
    assert r["seconds"]["0"]["fallback_s"] > 0
    # the given-multiplier twin of the entry: all ones gives the same words; a zero multiplier and a z0 element not below the modulus are invalid arguments
    assert r["ones"] == {"0": single, "2": single}
    assert r["codes"] == {"zero_multiplier": r["invalid"], "bad_z0": r["invalid"]} and r["invalid"] == _lib.ERR_INVALID


def test_the_nova_family_end_to_end(ivc):
    _family(ivc, last_bit=16, middle_bit=8)          # primary | secondary | fresh secondary


def test_the_cyclefold_family_end_to_end(cf):
    _family(cf, last_bit=8, middle_bit=16)           # U_n | u_n | cfU_n
