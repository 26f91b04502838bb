"""Many decider proofs under one key in one call, on the GPU (vimz_decider_verify_batch; vimz_amd/csrc/decider_batch.hip): the two new kernels through their hooks,
and the call end to end on the light decider of the hash step.

k_miller runs at n = 1, 2, 63, 64, 65 (PT_BLOCK is 64: half a wave's edge, a full block, a ragged second block) over the generators, P the identity, Q the identity,
P and −P against one Q and multiples, against tests/_miller_ref.py word for word — the restatement of the same projective formulas, which tests/test_miller_ref_host.py
ties to the pairing; the product of the values of P and −P is one after ONE final exponentiation.  k_g1_lincomb runs at the same n with a the identity, b the
identity, k = 0, k = r − 1 with a = b (the sum is the identity) and walks of 1, 128 and 254 bits, against tests/_pairing.py's g1_mul / g1_add.
End to end: three proofs of one prover at 2, 3 and 4 steps are accepted with chunk 0, 1 and 2; a batch of seven — the three and four tampered copies, one each for
the bits 2, 4, 8 and 16, placed so that chunks of two mix good and bad members — gives Decider.verify's bits for every member on the device path and on the host
path; two valid proofs with their C points swapped pass when every multiplier is one (the sums cannot see the swap) and are refused, bit 8 on both, by the
production entry, whose multipliers come from the OS.  The GPU half is tests/_decider_batch_gpu.py, a process per part."""
import json
import os
import subprocess
import sys

import pytest

from tests import _decider_batch_gpu as G
from tests import _miller_ref as M
from tests import _pairing as bp
from vimz_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_part(tmp_path_factory, part, timeout):
    out = tmp_path_factory.mktemp("decider_batch_" + part) / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._decider_batch_gpu", part, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return run_part(tmp_path_factory, "kernels", 600)


@pytest.fixture(scope="module")
def decider(tmp_path_factory):
    return run_part(tmp_path_factory, "decider", 900)


@pytest.fixture(scope="module")
def miller_expected():
    return [M.words(M.miller(q, p)) for p, q in G.miller_pairs()]


@pytest.fixture(scope="module")
def lincomb_expected():
    return [G.lincomb_expected(row) for row in G.lincomb_rows()]


@pytest.mark.parametrize("n", G.SIZES)
def test_the_miller_kernel_word_for_word(kernels, miller_expected, n):
    got = kernels["miller"][str(n)]
    assert len(got) == 96 * n
    for i in range(n):
        assert got[96 * i:96 * (i + 1)] == miller_expected[i], (n, i)


def test_the_miller_values_of_identities_and_of_opposite_points(kernels):
    got = kernels["miller"]["65"]
    one = [1] + [0] * 95
    assert got[96 * 1:96 * 2] == one and got[96 * 2:96 * 3] == one and got[0:96] != one
    f = M.f12_mul(M.from_words(got[96 * 3:96 * 4]), M.from_words(got[96 * 4:96 * 5]))           # e(P, Q)·e(−P, Q)
    assert f != M.F12_ONE and bp.final_exponentiate(M.to_pairing_basis(f)) == bp.F12_ONE
    assert kernels["bad_arguments"] == {"n_0": _lib.ERR_INVALID, "off_curve": _lib.ERR_INVALID, "bits_257": _lib.ERR_INVALID}


@pytest.mark.parametrize("n", G.SIZES)
def test_the_lincomb_kernel(kernels, lincomb_expected, n):
    got = [int(x) for x in kernels["lincomb"][str(n)]]
    for i in range(n):
        want = lincomb_expected[i]
        assert (got[2 * i], got[2 * i + 1]) == ((0, 0) if want is None else want), (n, i)
    if n >= 4:
        assert (got[6], got[7]) == (0, 0)                                                         # k = r − 1 with a = b: the identity


def test_three_proofs_of_one_prover_are_accepted(decider):
    assert decider["single"] == [0, 0, 0]
    assert decider["three"] == {"0": [0, 0, 0], "1": [0, 0, 0], "2": [0, 0, 0]}
    assert decider["empty"] == [] and "malformed key" in decider["bad_key"]


def test_a_batch_of_seven_gives_the_single_verifier_s_bits(decider):
    s = decider["seven"]
    assert s["single"] == [0, 2, 4, 0, 8, 0, 16] == s["key"]
    assert s["device"] == {"2": s["single"], "0": s["single"]} and s["host"] == s["single"]
    assert s["seconds"]["fallback"] > 1e-3 and s["seconds"]["miller_loops"] > 0


def test_swapped_c_points_pass_known_multipliers_and_not_the_os_s(decider):
    s = decider["swapped"]
    assert s["single"] == [8, 8] and s["restated_ones"] is True
    assert s["ones"] == [0, 0] and s["ones_host"] == [0, 0]
    assert s["production"] == [8, 8]
