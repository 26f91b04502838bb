"""The compressed proof's kernels (vimz_amd/csrc/spartan.hip: k_sum_partials, k_eq_step, k_sc_outer, k_sc_inner, k_bind, k_dot2, k_ipa_fold_vec,
k_ipa_fold_bases, k_combine3, k_committed_part, k_mask_public, the transposed sparse products and the loops around them) against the integer prover of
tests/_spartan_ref.py (checked on the CPU by tests/test_spartan_ref_host.py), through hooks that call the functions spartan_prove and ipa_prove run for every
round.  Every comparison is exact equality of words, and names the first message or element that differs; there is no tolerance anywhere.

Sum-checks, eq tables and the IPA's vector side on both fields at 2, 4, 8 elements, at half = 128, 256, 512 (half a block, one block, two partial sums into
k_sum_partials), on random, zero, p − 1 and unit vectors, strict and relaxed, u and single challenges at 0, 1, p − 1; the outer check and the vector folding
at 2^19 (the 512-block reductions stride) and the inner check and the eq table at 2^21 (the 2048-block streaming kernels stride), their inputs expanded from a
seed on both sides.  The generator folding on both curves around a wave and a block, at x = 0, 1, 2, 2^127, 2^128 − 1, with identities, a doubling and a
cancellation planted.  Whole instances, strict and relaxed on both curves, from 4 x 2 to 513 x 512 with every density class of the forward and transposed
products: the hook's bytes equal the integer prover's, both verifiers accept them and reject each of seven flipped bits and the instance with X0 + 1.

Wall time of this module on an MI355X: 16 s for its 81 tests, measured once (the probe process 4 s of them; the slowest tests are the striding cases at
1.6 – 2.1 s each, which is their integer reference on the host, not the kernels).  No test asserts a time."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest

from tests import _oracle
from tests import _spartan_kernels_gpu as P
from tests import _spartan_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = tmp_path_factory.mktemp("spartan_kernels") / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._spartan_kernels_gpu", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def orc():
    return _oracle.load()


def same(got_hex, want, what, names=None):
    """exact equality of words with the integers expected; names the first element (or message) that differs"""
    want_hex = P.ints_hex(want)
    if got_hex != want_hex:
        assert len(got_hex) == len(want_hex), f"{what}: {len(got_hex) // 64} elements, expected {len(want)}"
        k = next(i for i in range(len(want)) if got_hex[64 * i:64 * i + 64] != want_hex[64 * i:64 * i + 64])
        where = names(k) if names else f"element {k} of {len(want)}"
        raise AssertionError(f"{what}: {where} is {int.from_bytes(bytes.fromhex(got_hex[64 * k:64 * k + 64]), 'little')}, expected {want[k]}")


def same_rounds(got, msgs, finals, what, per, final_names):
    evals = {3: (0, 2, 3), 2: (0, 2)}[per] if final_names[0] != "a" else ("<a_L,b_R>", "<a_R,b_L>")
    same(got["msgs"], [x for m in msgs for x in m], what, lambda i: f"round {i // per}'s message at {evals[i % per]}")
    same(got["finals"], finals, what, lambda i: f"the bound value of {final_names[i]}")


def reference(kind, case, p):
    if kind == "outer":
        return S.outer_rounds(*case["vecs"], case["u"], S.from_list(case["chal"]), p)
    if kind == "inner":
        return S.inner_rounds(*case["vecs"], S.from_list(case["chal"]), p)
    return S.ipa_vec_rounds(*case["vecs"], S.from_list(case["chal"]), p)


SHAPE = {"outer": (3, ("eq", "Az", "Bz", "Cz", "E")), "inner": (2, ("M", "Z")), "ipa": (2, ("a", "b"))}


@pytest.mark.parametrize("k", S.SMALL_K)
@pytest.mark.parametrize("fid", [0, 1])
def test_eq_tables(probe, fid, k):
    for name in S.small_case_names("eq"):
        pt = S.small_case("eq", fid, k, name)["vecs"][0]
        same(probe["eq"][f"{fid}/{k}/{name}"], S.eq_table(pt, S.FIELD[fid]), f"eq table {name} of field {fid} at 2^{k}")


@pytest.mark.parametrize("k", S.SMALL_K)
@pytest.mark.parametrize("fid", [0, 1])
@pytest.mark.parametrize("kind", ["outer", "inner", "ipa"])
def test_rounds(probe, kind, fid, k):
    per, names = SHAPE[kind]
    for name in S.small_case_names(kind):
        case = S.small_case(kind, fid, k, name)
        msgs, fin = reference(kind, case, S.FIELD[fid])
        same_rounds(probe[kind][f"{fid}/{k}/{name}"], msgs, fin, f"{kind} rounds {name} of field {fid} at 2^{k}", per, names)


def test_outer_rounds_where_the_reductions_stride(probe):
    fid, k = S.OUTER_BIG
    u, chal = S.big_scalars("outer", fid, k)
    msgs, fin = S.outer_rounds(*[S.big_vector("outer", fid, k, w) for w in range(5)], u, S.from_list(chal), S.FIELD[fid])
    same_rounds(probe["outer"][f"{fid}/{k}/big"], msgs, fin, f"outer rounds at 2^{k}", *SHAPE["outer"])


def test_ipa_vector_rounds_where_the_reductions_stride(probe):
    fid, k = S.IPA_BIG
    _, chal = S.big_scalars("ipa", fid, k)
    dots, fin = S.ipa_vec_rounds(S.big_vector("ipa", fid, k, 0), S.big_vector("ipa", fid, k, 1), S.from_list(chal), S.FIELD[fid])
    same_rounds(probe["ipa"][f"{fid}/{k}/big"], dots, fin, f"IPA vector rounds at 2^{k}", *SHAPE["ipa"])


def test_inner_rounds_where_the_bind_strides(probe):
    fid, k = S.INNER_BIG
    _, chal = S.big_scalars("inner", fid, k)
    msgs, fin = S.inner_rounds(S.big_vector("inner", fid, k, 0), S.big_vector("inner", fid, k, 1), S.from_list(chal), S.FIELD[fid])
    same_rounds(probe["inner"][f"{fid}/{k}/big"], msgs, fin, f"inner rounds at 2^{k}", *SHAPE["inner"])


def test_eq_table_where_the_doubling_strides(probe):
    fid, k = S.EQ_BIG
    _, chal = S.big_scalars("eq", fid, k)
    tab = S.eq_table(chal, S.FIELD[fid])
    got = probe["eq"][f"{fid}/{k}/big"]
    for i in S.EQ_SAMPLES(1 << k):
        assert got["samples"][str(i)] == P.ints_hex([tab[i]]), f"eq table at 2^{k}: element {i}"
    want = [hashlib.sha256(b"".join(x.to_bytes(32, "little") for x in tab[i:i + S.EQ_CHUNK])).hexdigest() for i in range(0, len(tab), S.EQ_CHUNK)]
    assert len(got["digests"]) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got["digests"], want)) if g != w]
    assert not bad, f"eq table at 2^{k}: the first difference lies in elements [{bad[0] * S.EQ_CHUNK}, {(bad[0] + 1) * S.EQ_CHUNK})"


@pytest.mark.parametrize("cid", [0, 1])
def test_fold_bases(probe, cid):
    assert sorted(k for k in probe["fold"] if k.startswith(f"{cid}/")) == sorted(f"{cid}/{n}" for n in S.fold_case_names())
    for name in S.fold_case_names():
        pts, x = S.fold_case(cid, name)
        want = S.fold_bases(cid, pts, x)
        same(probe["fold"][f"{cid}/{name}"], [c for Pt in want for c in S.pt_words(Pt)], f"folded bases {name} on curve {cid}",
             lambda i: f"coordinate {'xy'[i % 2]} of point {i // 2}")
    at = S.PLANT["cancel"]
    assert probe["fold"][f"{cid}/planted/64"][128 * at:128 * at + 128] == "00" * 64          # the identity: sixteen zero words of 32 bits


@functools.lru_cache(maxsize=None)
def reference_bytes(name):
    return S.prove_instance(_oracle.load(), S.instance_case(name))


def test_every_case_is_in_the_probe(probe):
    assert sorted(probe["instance"]) == sorted(S.instance_names())
    for kind in ("eq", "outer", "inner", "ipa"):
        want = {f"{fid}/{k}/{name}" for fid in (0, 1) for k in S.SMALL_K for name in S.small_case_names(kind)}
        want.add("{}/{}/big".format(*{"eq": S.EQ_BIG, "outer": S.OUTER_BIG, "inner": S.INNER_BIG, "ipa": S.IPA_BIG}[kind]))
        assert set(probe[kind]) == want, kind
    assert set(probe["fold"]) == {f"{cid}/{n}" for cid in (0, 1) for n in S.fold_case_names()}


@pytest.mark.parametrize("name", S.instance_names())
def test_instance(probe, orc, name):
    case = S.instance_case(name)
    got = probe["instance"][name]
    blob, want = bytes.fromhex(got["blob"]), reference_bytes(name)
    # 1. the same bytes, message by message
    assert len(blob) == len(want) == 128 + S.argument_size(case)
    if blob != want:
        lay = sorted((off + 128, what) for what, off in S.argument_layout(case).items())
        k = next(i for i in range(0, len(want), 32) if blob[i:i + 32] != want[i:i + 32])
        near = [w for off, w in lay if off <= k]
        raise AssertionError(f"{name}: the element at byte {k} ({'the commitments' if k < 128 else 'at or after the ' + near[-1] if near else 'the outer messages'}) is "
                             f"{int.from_bytes(blob[k:k + 32], 'little')}, expected {int.from_bytes(want[k:k + 32], 'little')}")
    # 2., 3. both verifiers accept the hook's bytes
    assert S.verify_bytes(orc, case, blob) is None
    assert got["verify"] == 1
    # 4. and reject a flipped bit in each part of the argument (a strict instance has no E opening: six places)
    lay = S.argument_layout(case)
    assert set(got["tamper"]) == set(lay) and len(lay) == (7 if case["E"] is not None else 6)
    for what, off in lay.items():
        assert got["tamper"][what] == 0, f"{name}: the product's verifier accepted a flipped bit in the {what}"
        assert S.verify_bytes(orc, case, S.flip(blob, 128 + off)) is not None, f"{name}: the independent verifier accepted a flipped bit in the {what}"
    # 5. and the same proof for the instance with X0 + 1
    assert got["x0_plus_1"] == 0
    assert S.verify_bytes(orc, case, blob, X0_delta=1) is not None


def test_bad_arguments_are_refused(probe):
    assert {"eq_field", "eq_k_0", "eq_k_22", "eq_not_reduced", "sumcheck_field", "sumcheck_vector_not_reduced", "ipa_field", "ipa_not_reduced", "fold_curve",
            "fold_coordinate_not_reduced", "instance_curve", "instance_n_w_3", "instance_n_c_1", "instance_key_shorter_than_padded_shape"} <= set(probe["refused"])
    assert all(rc == probe["invalid"] for rc in probe["refused"].values()), probe["refused"]
    after = probe["accepted_after"]
    assert after["rc"] > 0 and after["same"] and after["eq"]          # a good call afterwards still succeeds, with the same words


def test_an_instance_proves_to_the_same_bytes_twice(probe):
    rep = probe["repeat"]
    assert rep["blobs"][0] == rep["blobs"][1] == probe["instance"][rep["name"]]["blob"]
