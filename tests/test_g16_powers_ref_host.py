"""tests/_g16_powers_ref.py — the decider's set-up from a powers-of-tau string on scalars — checked on the CPU before it judges a kernel: the Lagrange scalars by
inverse transform against the closed form; the derived key against decider_setup_impl's formulas on the trapdoor with gamma = 1; a three-row R1CS whose satisfying
assignment makes A(tau)·B(tau) − C(tau) = H(tau)·Z(tau) and the Groth16 equation hold in the exponent.  The cases laid out for the kernels are what they are meant to be."""
import pytest

from tests import _g16_powers_ref as P
from tests import _g16_ref as G
from tests._pairing import R

TAU, ALPHA, BETA, DELTA = 0x1234567890ABCDEF1234567, 0xFEDCBA987654321, 0x55AA55AA55AA77, 0x77665544332211FF


@pytest.mark.parametrize("logn", [1, 2, 3, 6, 9])
def test_lagrange_by_inverse_transform_is_the_closed_form(logn):
    s = P.string_scalars(TAU, ALPHA, BETA, logn)
    L = P.lagrange(s["tau_g1"], logn)
    assert L == P.lagrange_closed_form(TAU, logn)
    assert sum(L) % R == 1                                                       # the basis sums to one
    assert P.lagrange(s["alpha_g1"], logn) == [ALPHA * x % R for x in L] and P.lagrange(s["beta_g1"], logn) == [BETA * x % R for x in L]
    longer = P.string_scalars(TAU, ALPHA, BETA, logn + 1)                        # a longer string is used by its first powers
    assert P.lagrange(longer["tau_g1"], logn) == L


def three_row_r1cs():
    """wires (1, out, x, y, w), one public input: x·x = y, y·x = w, (w + x + 5)·1 = out"""
    dic = [1, 5, R - 1]
    A = ([0, 1, 2, 5], [2, 3, 4, 2, 0], [0, 0, 0, 0, 1])
    B = ([0, 1, 2, 3], [2, 2, 0], [0, 0, 0])
    Cm = ([0, 1, 2, 3], [3, 4, 1], [0, 0, 0])
    x = 3
    z = [1, x ** 3 + x + 5, x, x * x, x ** 3]
    return (A, B, Cm), dic, z, 5, 1, 3, 3                                           # matrices, dictionary, assignment, m, n_pub, n_c, logn


def rows_times(M, dic, z):
    row_ptr, col, coef = M
    return [sum(dic[coef[k]] * z[col[k]] for k in range(row_ptr[r], row_ptr[r + 1])) % R for r in range(len(row_ptr) - 1)]


def test_derived_key_is_the_trapdoor_key_with_gamma_one():
    mats, dic, z, m, n_pub, n_c, logn = three_row_r1cs()
    for power in (logn, logn + 1):
        got = P.derive_key(mats, dic, m, n_pub, n_c, logn, P.string_scalars(TAU, ALPHA, BETA, power), DELTA)
        assert got == P.trapdoor_key(mats, dic, m, n_pub, n_c, logn, TAU, ALPHA, BETA, 1, DELTA)
    with pytest.raises(AssertionError):
        P.derive_key(mats, dic, m, n_pub, n_c, logn, P.string_scalars(TAU, ALPHA, BETA, logn - 1), DELTA)


def test_three_row_r1cs_quotient_identity_and_groth16_equation():
    mats, dic, z, m, n_pub, n_c, logn = three_row_r1cs()
    n = 1 << logn
    az, bz, cz = (rows_times(M, dic, z) for M in mats)
    assert [x * y % R for x, y in zip(az, bz)] == cz                              # the assignment satisfies the rows
    a, b, c = (v + [0] * (n - n_c) for v in (az, bz, cz))
    for i in range(n_pub + 1):
        a[n_c + i] = z[i]
    h = G.quotient_pipeline(a, b, c, logn)
    assert h[n - 1] == 0
    key = P.derive_key(mats, dic, m, n_pub, n_c, logn, P.string_scalars(TAU, ALPHA, BETA, logn), DELTA)
    L = P.lagrange_closed_form(TAU, logn)
    At, Bt = G.dot(key["a"], z), G.dot(key["b"], z)
    Ct = G.dot(P.column_sums(mats[2], dic, m, L), z)
    HZ = DELTA * G.dot(h[:n - 1], key["h"]) % R
    assert HZ == G.horner(h, TAU) * (pow(TAU, n, R) - 1) % R
    assert (At * Bt - Ct) % R == HZ
    # Groth16 in the exponent (r = s = 0): (alpha + A)(beta + B) = alpha·beta + gamma·Σ_pub z_i ic_i + delta·(Σ_priv z_i l_i + Σ h_j hq_j)
    pub = G.dot(key["ic"], z[:n_pub + 1])
    priv = (G.dot(key["l"], z[n_pub + 1:]) + G.dot(h[:n - 1], key["h"])) % R
    assert (key["alpha"] + At) * (key["beta"] + Bt) % R == (key["alpha"] * key["beta"] + key["gamma"] * pub + key["delta"] * priv) % R
    z_bad = list(z); z_bad[1] += 1
    assert (key["alpha"] + G.dot(key["a"], z_bad)) * (key["beta"] + Bt) % R != (key["alpha"] * key["beta"] + G.dot(key["ic"], z_bad[:n_pub + 1]) + key["delta"] * priv) % R


def test_kernel_cases_are_what_they_are_meant_to_be():
    for group, logns in P.TRANSFORM_LOGN.items():
        assert {1, 2, 3} <= set(logns) and any((1 << logn) // 2 == P.PT_BLOCK for logn in logns)
    assert {(1 << logn) // 2 for logn in P.TRANSFORM_LOGN[1]} >= {P.PT_BLOCK // 2, P.PT_BLOCK, 2 * P.PT_BLOCK}
    c = P.transform_cases(3)
    assert c["half_period"][:4] == c["half_period"][4:] and 0 in c["holes"] and any(c["holes"]) and len(set(c["constant"])) == 1
    e = P.transform_expected(c["constant"], 3, "random")
    assert set(P.transform_expected(c["constant"], 3, "constant")) == {"fwd"} and set(P.FULL_CASES) <= set(c)
    assert e["fwd"][0] == 8 * c["constant"][0] % R and not any(e["fwd"][1:])      # every output but the first is the identity
    assert P.transform_expected(c["e_1"], 3, "e_1")["fwd"] == [pow(G.omega(3), i, R) for i in range(8)]
    assert e["inv_scaled"] == P.lagrange(c["constant"], 3)
    dic = P.coefficients()
    assert {1, R - 1, 2, 0} <= set(dic) and any(x > 1 << 250 for x in dic) and any(x == 1 << k for x in dic for k in (17, 200)) and any(R - x == 1 << 200 for x in dic)
    case = P.colsum_case(65)
    row_ptr, col, coef = case["csr"]
    lengths = [col.count(j) for j in range(65)]
    assert lengths[:7] == [P.COL_SPLIT - 1, P.COL_SPLIT, P.COL_SPLIT + 1, 0, 1, P.COL_CHUNK + 1, P.COL_CHUNK]
    want = P.colsum_expected(case)
    s = case["scalars"]
    assert want[7] == 2 * s[0] % R and want[8] == 0 and want[9] == s[5] and want[11] == 3 * s[0] % R and want[3] == 0
    assert 0 in s and s[0] == s[1] and (s[0] + s[2]) % R == 0
    assert not any(P.colsum_expected(P.colsum_case(64, "empty"))) and P.colsum_case(64, "empty")["csr"][0] == [0] * (case["n_rows"] + 1)
    assert set(P.colsum_cases()) >= {f"{n}/mixed" for n in P.COLSUM_COLS} | {f"1/{k}" for k in (0, 1, 31, 32, 33)}
    assert set(P.SCALE_N) == {P.PT_BLOCK - 1, P.PT_BLOCK, P.PT_BLOCK + 1} and 0 in P.scale_points(64)
    assert set(P.scale_scalars().values()) >= {1, 2, R - 1}


def test_kzg_from_powers_judges_the_string_before_it_touches_a_gpu():
    """hip.kzg_from_powers' refusals need no context: n below 2 or beyond the string, a single power in G2, a first power that is not the generator, a coordinate
    of tau_g2[1] that is not below q — each VimzError(ERR_INVALID), over a `.ptau` container read back by iden3.read_ptau."""
    import numpy as np
    from tests.test_ptau_host import string_of, write_ptau
    from tests._pairing import Q
    from vimz_amd import _lib, hip, iden3
    powers = iden3.read_ptau(write_ptau(1, string_of(1)))
    big = np.array(powers["tau_g2"])
    big[1, 4:8] = np.frombuffer(Q.to_bytes(32, "little"), dtype="<u8")
    for bad, n in ((powers, 1), (powers, 0), (powers, 4), (dict(powers, tau_g2=powers["tau_g2"][:1]), 2), (dict(powers, tau_g1=powers["tau_g1"][1:]), 2),
                   (dict(powers, tau_g2=big), 2)):
        with pytest.raises(_lib.VimzError) as e:
            hip.kzg_from_powers(None, bad, n)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(AttributeError):      # a good string gets as far as the context
        hip.kzg_from_powers(None, powers, 3)
