"""The Python statement of further delta contributions to a saved decider key (tests/_key_contrib_ref.py: the blob's parser, contribute, the record and its
challenge, the whole verdict of vimz_decider_key_verify_contributions) on synthetic keys whose points are [s]G for known scalars — m = 6, n_pub = 1, n = 4, and one with
an identity in l; the layout is read from the header, so they belong to no circuit.  Chains of 0, 1 and 3 records are accepted, every tamper yields exactly its bits
and its first_bad, and contribute(key(delta), delta') is key(delta·delta') byte for byte.  The GPU tests (tests/test_gpu_key_contrib.py) compare the library with it."""
import os

import pytest

from tests import _key_contrib_ref as K
from tests._pairing import Q, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LH = 7


def rho():
    return K.fixed_rho(N_LH)


def test_the_layout_is_read_from_the_header():
    key = K.synthetic_key(K.DELTA0)
    L = K.layout(key)
    assert (L["m"], L["n_pub"], L["n"], L["n_lh"]) == (6, 1, 4, N_LH) and 8 * L["words"] == len(key)
    assert L["off_lh"] == K.KEY_IC + 8 * 2 + 16 * 6 and K.KEY_MAGIC == 0x3259454B36314756 and K.RECORD_MAGIC == 0x3152544336314756
    assert K.g1_at(key, K.KEY_DELTA1) == K.bp.g1_mul(K.bp.G1, K.DELTA0) and K.g2_at(key, K.KEY_DELTA2) == K.bp.g2_mul(K.bp.G2, K.DELTA0)
    huge = K.put(key, 1, (1 << 40).to_bytes(8, "little"))            # a header that names sizes the blob does not have
    for blob, msg in ((key[:-8], "wrong length"), (key + bytes(8), "wrong length"), (key[:-1], "not a decider key"), (key[:8 * K.KEY_IC - 8], "not a decider key"),
                      (K.put(key, 0, b"VG16KEY1"), "not a decider key"), (huge, "not a decider key"), (K.put(key, 2, (6).to_bytes(8, "little")), "not a decider key"), (b"", "not a decider key")):
        with pytest.raises(ValueError, match=msg):
            K.layout(blob)


@pytest.mark.parametrize("identity", (None, 2))
def test_a_contribution_is_the_key_of_the_product(identity):
    key = K.synthetic_key(K.DELTA0, K.SMALL, identity)
    out, rec = K.contribute(key, K.DELTAS[0], K.NONCES[0])
    assert out == K.synthetic_key(K.DELTA0 * K.DELTAS[0] % R, K.SMALL, identity)
    assert len(rec) == K.RECORD_BYTES and int.from_bytes(rec[:8], "little") == K.RECORD_MAGIC
    # the record: delta1, delta2 after; T = k·delta1_before; z = k + c·delta'
    assert rec[8:72] == out[8 * K.KEY_DELTA1:8 * K.KEY_DELTA1 + 64] and rec[72:200] == out[8 * K.KEY_DELTA2:8 * K.KEY_DELTA2 + 128]
    assert K.g1_at(rec, K.REC_T) == K.bp.g1_mul(K.bp.G1, K.DELTA0 * K.NONCES[0] % R)
    c = K.challenge(key[:88], key[8 * K.KEY_DELTA1:8 * K.KEY_DELTA1 + 64], rec)
    assert c < 1 << 248 and K.coord(rec, K.REC_Z) == (K.NONCES[0] + c * K.DELTAS[0]) % R
    assert K.knowledge_holds(key[:88], K.g1_at(key, K.KEY_DELTA1), rec)
    other_head = K.put(key, 7, (5).to_bytes(32, "little"))[:88]      # a record is bound to the key's header and pp_hash
    assert not K.knowledge_holds(other_head, K.g1_at(key, K.KEY_DELTA1), rec)


@pytest.mark.parametrize("n_records", (0, 1, 3))
def test_chains_are_accepted(n_records):
    origin, final, records = K.chain(K.SMALL, n_records)
    assert len(records) == n_records * K.RECORD_BYTES
    assert K.verify(origin, final, records, rho()) == (0, (0, 0))


def test_a_chain_over_an_identity_in_l_is_accepted():
    origin, final, records = K.chain(K.SMALL, 1, 2)
    assert K.lh_points(origin)[2] == (0, 0) == K.lh_points(final)[2]
    assert K.verify(origin, final, records, rho()) == (0, (0, 0))


@pytest.mark.parametrize("name", sorted(K.tamper_table()))
def test_a_tampered_chain_yields_its_bits(name):
    assert K.verify(*K.tampered_chains()[name], rho()) == K.tamper_table()[name]


def test_the_tampers_cover_every_bit_but_the_subgroup():
    seen = 0
    for bits, _first in K.tamper_table().values():
        seen |= bits
    assert seen == K.COORD | K.OFF_CURVE | K.IDENTITY | K.FIXED_PART | K.DELTA_HALVES | K.KNOWLEDGE | K.LAST | K.RATIO


def test_a_delta2_outside_the_subgroup_is_named():
    from tests._powers_verify_ref import outside_points
    origin, final, records = K.chain(K.SMALL, 1)
    bad = K.put(records, K.REC_DELTA2, K.g2_bytes(outside_points()["mixed"]))
    assert K.verify(origin, final, bad, rho()) == (K.SUBGROUP, (K.AT_RECORD, 0))


def test_keys_of_other_sizes_differ_in_their_fixed_part():
    origin, _final, records = K.chain(K.SMALL, 1)
    assert K.verify(origin, K.synthetic_key(K.DELTA0, K.LARGE), records, rho()) == (K.FIXED_PART, (K.AT_FIXED_PART, 1))


def test_malformed_input_is_an_error_not_a_verdict():
    origin, final, records = K.chain(K.SMALL, 1)
    for args in ((origin[:-8], final, records), (origin, final + bytes(8), records), (origin, final, records[:-8]), (origin, final, K.put(records, 0, b"VG16CTR2"))):
        with pytest.raises(ValueError):
            K.verify(*args, rho())


@pytest.mark.parametrize("name", K.REFUSED_KEYS)
def test_contribute_refuses(name):
    blob, msg = K.refused_keys()[name]
    with pytest.raises(ValueError, match=msg):
        K.contribute(blob, K.DELTAS[0], K.NONCES[0])


def test_the_combinations_cases_hold_what_they_promise():
    cases = K.ratio_cases()
    assert {int(name.split("/")[0]) for name in cases} == set(K.RATIO_SIZES) | {2}
    b, a, r = cases[f"{K.PT_BLOCK * K.RLC_CHUNK + 1}/multiple"]
    assert len(b) == 513 and b[2] == 0 == a[2] and r[3] == 0 and r[4] == K.MAX128 and b[5] == b[6] and r[5] == r[6]
    chunks = K.ratio_chunk_scalars(b, r)
    assert len(chunks) == K.PT_BLOCK + 1 and chunks[1] == 0 and chunks[0] and chunks[-1]            # a chunk that cancels; a last chunk of one point
    assert all(x == 5 * y % R for x, y in zip(a, b))
    b, a, r = cases["19/unrelated"]
    assert K.ratio_scalars(b, a, r)[1] != 5 * K.ratio_scalars(b, a, r)[0] % R
    assert K.ratio_scalars(*cases["2/whole_sum_identity"]) == (0, 0)


def test_the_constants_are_the_librarys():
    hpp = open(os.path.join(ROOT, "vimz_amd", "csrc", "g16_key_contrib.hpp")).read()
    assert f"KEY_HEAD_WORDS = {K.KEY_HEAD_WORDS}, KEY_DELTA1 = {K.KEY_DELTA1}, KEY_DELTA2 = {K.KEY_DELTA2}, KEY_IC = {K.KEY_IC};" in hpp
    assert f"RECORD_WORDS = {K.RECORD_WORDS}, REC_DELTA1 = {K.REC_DELTA1}, REC_DELTA2 = {K.REC_DELTA2}, REC_T = {K.REC_T}, REC_Z = {K.REC_Z};" in hpp
    assert f'RECORD_TAG[] = "{K.TAG.decode()}";' in hpp and f"RECORD_MAGIC = 0x{K.RECORD_MAGIC:x}ull" in hpp
    hdr = open(os.path.join(ROOT, "include", "vimz_hip.h")).read()
    for k, name in enumerate(("COORD", "OFF_CURVE", "IDENTITY", "SUBGROUP", "FIXED_PART", "DELTA_HALVES", "KNOWLEDGE", "LAST", "RATIO")):
        assert f"#define VIMZ_KEYCHAIN_{name} 0x{1 << k:x}u" in hdr and getattr(K, name) == 1 << k, name
    for k, name in enumerate(("ORIGIN_DELTA", "FINAL_DELTA", "RECORD", "ORIGIN_LH", "FINAL_LH", "FIXED_PART"), 1):
        assert f"#define VIMZ_KEYCHAIN_AT_{name} {k}\n" in hdr and getattr(K, "AT_" + name) == k, name
    from vimz_amd import hip
    assert set(hip.KEYCHAIN_BITS) == {1 << k for k in range(9)} and len(hip.KEYCHAIN_PLACES) == 7
    assert Q > R
