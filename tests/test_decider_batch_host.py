"""vimz_decider_verify_batch without a GPU (ctx = None: every device stage as the host's loop over the kernels' per-thread functions; vimz_amd/csrc/decider_batch.hpp,
pairing_stage.hpp, decider_verify.hpp) on the reference's six committed proofs with the constants of contracts/*Verifier.sol as keys: each proof alone, copies of one
proof over several chunks, and copies with one word changed beside good ones — every result the bits vimz_decider_verify_key gives for that proof alone.

tests/native/decider_batch_check.cpp, built with g++ -fsanitize=address,undefined and run directly, loops g1_lincomb_thread and miller_thread over every index at
n = 1, 2, 65 from heap blocks of exact size — checking after every thread that it wrote its own slot and no other — and runs the host batch path on a synthetic key
whose trapdoor it knows.  Here its words against tests/_miller_ref.py and tests/_pairing.py."""
import os
import subprocess

import pytest

from tests import _miller_ref as M
from tests import _novadecider as nd
from tests import _pairing as bp
from tests.test_novadecider import CONTRACT_OF, _statement
from vimz_amd import _lib
from vimz_amd.hip import decider_verify_key, verify_decider_batch, verifying_key_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, R = bp.Q, bp.R


@pytest.fixture(scope="module")
def keys():
    return nd.verifier_keys()


@pytest.mark.parametrize("name", sorted(CONTRACT_OF))
def test_each_committed_proof_alone_is_accepted(keys, name):
    kw = verifying_key_words(keys[CONTRACT_OF[name]])
    sec = {}
    assert verify_decider_batch(None, kw, [_statement(name)], seconds=sec) == [0]
    assert sec["fallback"] < 1e-3 < sec["total"]            # accepted by the product, not by the single verifier behind it (one verification there takes 0.03 s)


def test_copies_of_one_proof_over_two_chunks_are_accepted(keys):
    kw = verifying_key_words(keys["contrast"])
    assert verify_decider_batch(None, kw, [_statement("img2-contrast")] * 3, chunk=2) == [0, 0, 0]
    assert verify_decider_batch(None, kw, []) == []


def test_a_changed_word_of_each_kind_gives_the_single_verifier_s_bits(keys):
    steps, z0, zf, words = _statement("img2-contrast")
    kw = verifying_key_words(keys["contrast"])

    def changed(at, fn):
        w = list(words)
        w[at] = fn(w[at])
        return (steps, z0, zf, w)

    items = [(steps, z0, zf, words),
             changed(10, lambda v: Q - v),                                  # an A word: −A
             changed(19, lambda v: (v + 1) % R),                            # a KZG evaluation
             (steps, z0, zf[:-1] + [R + 5], words),                         # a z_i not below r
             changed(4, lambda v: v ^ 1),                                   # u_i.cmW off the curve
             (1, z0, zf, words),                                            # steps = 1
             (steps, z0, zf, words)]
    want = [decider_verify_key(kw, *it) for it in items]
    assert want[0] == 0 and want[1] == 8 and want[2] & 2 and want[3] == 8 and want[4] == 16 and want[5] & 1 and want[6] == 0
    for chunk in (0, 2, 1):
        sec = {}
        assert verify_decider_batch(None, kw, items, chunk=chunk, seconds=sec) == want, chunk
        assert sec["fallback"] > 1e-3
    # a B that is on the twist's curve but not in the subgroup is malformed; here: B's parts swapped, off the twist
    w = list(words); w[11], w[12], w[13], w[14] = w[12], w[11], w[14], w[13]
    assert verify_decider_batch(None, kw, [(steps, z0, zf, w), (steps, z0, zf, words)]) == [16, 0]


def test_bad_arguments_are_refused_with_a_message(keys):
    steps, z0, zf, words = _statement("img2-contrast")
    kw = verifying_key_words(keys["contrast"])
    for bad_kw, item in ((kw[:-1], (steps, z0, zf, words)), (kw, (steps, z0[:2], zf[:2], words))):
        with pytest.raises(_lib.VimzError) as e:
            verify_decider_batch(None, bad_kw, [item])
        assert "vimz_decider_verify_batch" in str(e.value)


# ---- the native program ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = tmp_path_factory.mktemp("decider_batch") / "decider_batch_check"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "vimz_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "decider_batch_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_cpu_loop_of_the_miller_kernel_is_the_restated_formulas(native):
    seen = 0
    for label, toks in native.items():
        if not label.startswith("miller/"):
            continue
        i = int(label.split("/")[2])
        p = None if i % 7 == 1 else bp.g1_mul(bp.G1, 3 + 5 * i)
        q = None if i % 7 == 2 else bp.g2_mul(bp.G2, 7 + 11 * i)
        want = [c for k in M.STRUCT_ORDER for c in M.miller(q, p)[k]]
        assert [int(t, 16) for t in toks] == want, label
        seen += 1
    assert seen == 1 + 2 + 7 and native["miller/65/64"] != native["miller/65/63"]
    assert [int(t, 16) for t in native["miller/2/1"]] == [1] + [0] * 11             # P the identity: one


def test_cpu_loop_of_the_lincomb_kernel(native):
    seen = 0
    for label, toks in native.items():
        if not label.startswith("lincomb/"):
            continue
        i = int(label.split("/")[2])
        bits, k, x, y = int(toks[0]), int(toks[1], 16), int(toks[2], 16), int(toks[3], 16)
        a, b = bp.g1_mul(bp.G1, 1000 + i), bp.g1_mul(bp.G1, 2000 + 3 * i)
        if i == 0:
            a = None
        elif i == 1:
            b = None
        elif i == 2:
            assert k == 0
        elif i == 3:
            a = b
            assert k == R - 1 and bits == 254
        want = bp.g1_add(a, None if b is None else bp.g1_mul(b, k & ((1 << bits) - 1)))
        assert (x, y) == ((0, 0) if want is None else want), label
        seen += 1
    assert seen == 1 + 2 + 10 and native["lincomb/65/3"][2:] == ["0" * 64] * 2
    assert {int(native[f"lincomb/65/{i}"][0]) for i in (4, 5, 6)} == {1, 128, 254}


def test_the_host_batch_path_on_a_synthetic_key(native):
    pairs = lambda name: [tuple(int(v) for v in t.split(":")) for t in native[f"batch/{name}"][1:]]      # noqa: E731
    for name in ("good", "one_chunk", "mixed", "noncanonical", "swapped", "none"):
        assert native[f"batch/{name}"][0] == "0" and all(got == want for got, want in pairs(name)), name
    assert [w for _, w in pairs("mixed")] == [0, 2 | 8, 8, 16, 1 | 8] and [w for _, w in pairs("noncanonical")][0] == 8
    # two proofs with their C points swapped: each refused alone; the sums cannot see the swap when every multiplier is one, the OS's multipliers do
    assert pairs("swapped_ones") == [(0, 8), (0, 8)] and pairs("swapped") == [(8, 8), (8, 8)]
    assert native["batch/zero_multiplier"][0] != "0"


# ---- the restated formulas themselves --------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_header_s():
    src = open(os.path.join(ROOT, "vimz_amd", "csrc", "pairing_stage.hpp")).read()
    assert f"ATE_LOW = {M.ATE_LOW}ull" in src and (1 << 64) + M.ATE_LOW == bp.ATE_LOOP_COUNT
