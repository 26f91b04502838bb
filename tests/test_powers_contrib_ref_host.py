"""tests/_powers_contrib_ref.py against itself, without a GPU: a contribution of (tau', alpha', beta') to the string of (tau, alpha, beta) is the string of
(tau·tau', alpha·alpha', beta·beta') — on scalars at every power the GPU tests use and on points at the smallest —, the record's proofs hold over the right
base and fail over another, chains are accepted, and every tamper of the table yields the bits the table states."""
import pytest

from tests import _g16_powers_ref as P
from tests import _powers_contrib_ref as K
from tests import _powers_verify_ref as V
from tests._pairing import R


@pytest.mark.parametrize("power", K.POWERS)
def test_a_contribution_on_scalars_is_the_string_of_the_products(power):
    strings = K.chain_scalars(power, 3)
    tau, alpha, beta = K.TAU0, K.ALPHA0, K.BETA0
    for j in range(3):
        tp, ap, bp_ = K.SECRET_SETS[j]
        tau, alpha, beta = tau * tp % R, alpha * ap % R, beta * bp_ % R
        assert strings[j + 1] == P.string_scalars(tau, alpha, beta, power), j
        assert K.triple(strings[j + 1]) == (tau, alpha, beta)
    assert len(strings[0]["tau_g1"]) == 2 * (1 << power) - 1


def test_a_contribution_on_points_is_the_contribution_on_scalars():
    s0, s1 = K.chain_scalars(1, 1)
    got, rec = K.contribute_points(V.string_points(s0), K.SECRET_SETS[0], K.NONCE_SETS[0])
    assert got == V.string_points(s1)
    assert rec == K.chain_records(1)
    assert K.record_points(rec)[0] == K.base_points(got)
    assert K.knowledge_failed(K.base_points(V.string_points(s0)), rec) == 0
    assert K.knowledge_failed(K.base_points(got), rec) == 7                     # over another base every proof fails
    assert V.judge(got, K.fixed_rho(2)) == (0, (0, 0))


def test_contribute_refuses_with_its_message():
    assert set(K.refused_strings()) == set(K.REFUSED_STRINGS)
    for name, string in K.refused_strings().items():
        with pytest.raises(ValueError, match=K.REFUSED_STRINGS[name].replace("[", ".").replace("]", ".")):
            K.contribute_points(string, K.SECRET_SETS[0], K.NONCE_SETS[0])


@pytest.mark.parametrize("n_records", (0, 1, 3))
def test_chains_are_accepted(n_records):
    assert K.verify(*K.chain(K.TAMPER_POWER, n_records)) == (0, 0, (0, 0))


def test_a_chain_from_the_new_string_is_accepted():
    strings = K.chain_scalars(1, 2, new=True)
    assert K.triple(strings[0]) == (1, 1, 1) and set(strings[0]["tau_g1"]) == {1}
    assert K.verify(K.scalar_points((1, 1, 1)), V.string_points(strings[-1]), K.chain_records(2, new=True)) == (0, 0, (0, 0))
    assert K.verify(K.scalar_points((1, 1, 1)), V.string_points(strings[0]), b"") == (0, 0, (0, 0))      # worthless, and a string


@pytest.mark.parametrize("name", sorted(K.tamper_table()))
def test_a_tampered_chain_yields_the_tables_bits(name):
    assert K.verify(*K.tampered_chains()[name]) == K.tamper_table()[name], name


def test_the_tampers_asked_for_are_all_there():
    assert set(K.tamper_table()) == ({f"record_{part}/{s}" for part in "ATz" for s in K.SECRETS} | {f"final_point/{a}" for a in V.ARRAYS[1:]}
                                     | {"records_swapped", "last_record_dropped", "middle_record_dropped", "last_record_of_another_string", "final_point_off_curve",
                                        "record_point_identity", "record_point_off_curve", "origin_coordinate_is_q"})


def test_records_that_are_no_records():
    origin, final, records = K.chain()
    with pytest.raises(ValueError, match="488 bytes"):
        K.verify(origin, final, records[:-1])
    with pytest.raises(ValueError, match="record 1 is not"):
        K.verify(origin, final, K.put(records, K.RECORD_WORDS, b"VG16CTR1"))


def test_the_kernel_cases_cover_what_they_should():
    assert [K.bitlen_of_count(c) for c in K.POWER_COUNTS] == [0, 1, 2, 6, 6, 7, 8, 11]
    assert (1 << 250) <= K.POWER_WS["random"] < R and K.POWER_WS["r_minus_1"] == R - 1
    for group, sizes in K.SCALE_N.items():
        cases = K.scale_cases(group)
        assert len(cases) == 7 * len(sizes)
        for n in sizes:
            s = K.scale_inputs(n)
            assert s[0] == 0 == s[n // 2] and (n == 1 or all(s[1:n // 2]))
            want = K.scale_expected(s, R - 1, 1)                                # the scalars alternate between 1 and r − 1
            assert all(w == (x if k % 2 == 0 else R - x) % R for k, (w, x) in enumerate(zip(want, s)))
            assert K.scale_expected(s, 1, 1) == s and not any(K.scale_expected(s, K.W_RANDOM, 0))
