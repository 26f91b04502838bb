"""tests/_miller_ref.py — the restatement of k_miller's projective Miller loop and of vimz_decider_verify_batch's equation — against tests/_pairing.py, which the
CPU suite pins on the reference's six committed proofs: a Miller value of the restatement, mapped into _pairing's basis and raised by its final exponentiation,
is _pairing's pairing (the two Miller values differ by factors in Fq2, which the exponentiation removes); the pairing is bilinear; the batch equation accepts
committed proofs and refuses a changed one.  Final exponentiations in this file: nine."""
import pytest

from tests import _miller_ref as M
from tests import _novadecider as nd
from tests import _pairing as bp
from tests.test_novadecider import _statement


def gt(q2, p1):
    return bp.final_exponentiate(M.to_pairing_basis(M.miller(q2, p1)))


@pytest.mark.parametrize("a,b", [(1, 1), (0x1F2E3D4C5B6A7988, 0xABCDEF0123456789ABCDEF), (bp.R - 2, 3)])
def test_the_restated_miller_value_gives_the_pairing(a, b):
    p, q = bp.g1_mul(bp.G1, a), bp.g2_mul(bp.G2, b)
    f = M.miller(q, p)
    assert gt(q, p) == bp.pairing(q, p) != bp.F12_ONE                              # 2 exponentiations a case
    assert M.to_pairing_basis(f) != bp.miller_loop(q, p)                           # ... and not because the two Miller values are the same
    assert M.from_words(M.words(f)) == f and len(M.words(f)) == 96


def test_bilinearity_and_the_identities():
    p, q = bp.g1_mul(bp.G1, 5), bp.g2_mul(bp.G2, 7)
    assert M.miller(None, p) == M.miller(q, None) == M.F12_ONE
    f = M.f12_mul(M.miller(q, p), M.miller(bp.G2, bp.g1_neg(bp.g1_mul(bp.G1, 35))))   # e(5P, 7Q)·e(−35P, Q)
    assert bp.final_exponentiate(M.to_pairing_basis(f)) == bp.F12_ONE               # 1


def test_the_basis_map_is_a_ring_map():
    f, g = M.miller(bp.G2, bp.G1), M.miller(bp.g2_mul(bp.G2, 2), bp.G1)
    assert M.to_pairing_basis(M.f12_mul(f, g)) == bp.f12_mul(M.to_pairing_basis(f), M.to_pairing_basis(g))
    assert M.to_pairing_basis(M.F12_ONE) == bp.F12_ONE


def test_the_batch_equation_on_committed_proofs():
    """two copies of a committed proof under distinct multipliers: accepted; with one evaluation changed: refused (2 exponentiations)"""
    key = nd.verifier_keys()["contrast"]
    steps, z0, zf, words = _statement("img2-contrast")
    good = (steps, z0, zf, words)
    sc = [(3, 5, 7), (0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321FEDCBA0987654321, 1 << 127)]
    assert M.batch_accepts(key, [good, good], sc)
    bad = list(words); bad[19] = (bad[19] + 1) % bp.R
    assert not M.batch_accepts(key, [good, (steps, z0, zf, bad)], sc)
