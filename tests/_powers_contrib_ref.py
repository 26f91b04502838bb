"""A contribution to a powers-of-tau string and the check of a chain of them (vimz_powers_contribute / vimz_powers_verify_contributions; vimz_amd/csrc/
g16_powers_contrib.hip and .hpp) stated in plain Python integers: the contribution on SCALARS (a point [s]G is its s; on tests/_g16_powers_ref.string_scalars' strings)
and on points over tests/_pairing.py's arithmetic, the record and its three challenges, the whole verdict — and the chains, tampered chains and kernel cases the CPU
tests (tests/test_powers_contrib_ref_host.py, tests/test_powers_contrib_host.py) and the GPU tests (tests/test_gpu_powers_contrib.py) run.  A string of points is
tests/_powers_verify_ref.string_points' dictionary (the identity as zeros).  No GPU, no numpy.  Test infrastructure."""
import functools
import hashlib
import random

from tests import _g16_powers_ref as P
from tests import _pairing as bp
from tests import _powers_verify_ref as V
from tests._key_contrib_ref import coord, dec1, g1_at, g1_bytes, put
from tests._pairing import Q, R

RECORD_MAGIC = int.from_bytes(b"VPOTCTR1", "little")
RECORD_WORDS, RECORD_BYTES = 61, 488
REC_A, REC_T, REC_Z = 1, 25, 49                                # word offsets of a record (g16_powers_contrib.hpp)
TAG = b"vimz-powers-of-tau-contribution"
COORD, OFF_CURVE, IDENTITY, KNOWLEDGE_TAU, KNOWLEDGE_ALPHA, KNOWLEDGE_BETA, LAST, STRING = (1 << k for k in range(8))      # VIMZ_POWCHAIN_*
KNOWLEDGE = (KNOWLEDGE_TAU, KNOWLEDGE_ALPHA, KNOWLEDGE_BETA)
KNOWLEDGE_ALL = KNOWLEDGE_TAU | KNOWLEDGE_ALPHA | KNOWLEDGE_BETA
AT_ORIGIN, AT_RECORD = 1, 2                                    # VIMZ_POWCHAIN_AT_*; _AT_STRING_<array> = AT_RECORD + vimz_powers_verify's array number
SECRETS = ("tau", "alpha", "beta")
PT_BLOCK = 64


# ---- the contribution on scalars and on points ---------------------------------------------------------------------------------------------------------
def contribute_scalars(s, tau_p, alpha_p, beta_p):
    """the string of scalars after a contribution: tau_g1[k], tau_g2[k] times tau'^k, alpha_g1[k] times alpha'·tau'^k, beta_g1[k] times beta'·tau'^k, beta_g2 times beta'"""
    pw = [pow(tau_p, k, R) for k in range(len(s["tau_g1"]))]
    return {"power": s["power"], "tau_g1": [x * w % R for x, w in zip(s["tau_g1"], pw)], "tau_g2": [x * w % R for x, w in zip(s["tau_g2"], pw)],
            "alpha_g1": [x * w * alpha_p % R for x, w in zip(s["alpha_g1"], pw)], "beta_g1": [x * w * beta_p % R for x, w in zip(s["beta_g1"], pw)],
            "beta_g2": [s["beta_g2"][0] * beta_p % R]}


def base_points(string):
    """the three points a record is made over: tau_g1[1], alpha_g1[0], beta_g1[0]"""
    return [string["tau_g1"][1], string["alpha_g1"][0], string["beta_g1"][0]]


def contribute_points(string, secrets, nonces):
    """(string, record) after a contribution on POINTS, one multiplication a point as the kernel does it; ValueError with vimz_powers_contribute's message"""
    for name in V.ARRAYS[1:]:
        if any(max(V.flat(V.GROUP[name], p)) >= Q for p in string[name]):
            raise ValueError("a coordinate is not below q")
    for name in V.ARRAYS[1:]:
        on = bp.g1_on_curve if V.GROUP[name] == 1 else bp.g2_on_curve
        if not all(on(V.dec(V.GROUP[name], p)) for p in string[name]):
            raise ValueError("a point is not on its curve")
    if any(dec1(p) is None for p in base_points(string)):
        raise ValueError("tau_g1[1], alpha_g1[0] or beta_g1[0] is the identity")
    tau_p, alpha_p, beta_p = secrets
    m1 = lambda p, k: V.enc(1, bp.g1_mul(V.dec(1, p), k))      # noqa: E731
    m2 = lambda p, k: V.enc(2, V.g2_mul_raw(V.dec(2, p), k % R))      # noqa: E731
    out = {"tau_g1": [m1(p, pow(tau_p, k, R)) for k, p in enumerate(string["tau_g1"])], "tau_g2": [m2(p, pow(tau_p, k, R)) for k, p in enumerate(string["tau_g2"])],
           "alpha_g1": [m1(p, alpha_p * pow(tau_p, k, R)) for k, p in enumerate(string["alpha_g1"])],
           "beta_g1": [m1(p, beta_p * pow(tau_p, k, R)) for k, p in enumerate(string["beta_g1"])], "beta_g2": [m2(string["beta_g2"][0], beta_p)]}
    return out, make_record(base_points(string), secrets, nonces)


# ---- the record ----------------------------------------------------------------------------------------------------------------------------------------
def points_bytes(points):
    return b"".join(g1_bytes(dec1(p)) for p in points)


def challenge(which, before, record):
    """c of secret `which` (0 tau', 1 alpha', 2 beta'): before = B_tau ‖ B_alpha ‖ B_beta, 192 bytes; SHA3-256 read as groth16.hip's fr_from_hash reads a digest"""
    d = hashlib.sha3_256(TAG + which.to_bytes(8, "little") + before + record[8 * REC_A:8 * REC_T] + record[8 * (REC_T + 8 * which):8 * (REC_T + 8 * which + 8)]).digest()
    return int.from_bytes(d[:31], "little")


def make_record(before, secrets, nonces):
    """the record over the points before = [B_tau, B_alpha, B_beta]"""
    rec = RECORD_MAGIC.to_bytes(8, "little") + points_bytes([bp.g1_mul(dec1(b), s) for b, s in zip(before, secrets)]) + points_bytes([bp.g1_mul(dec1(b), k) for b, k in zip(before, nonces)])
    bb = points_bytes(before)
    return rec + b"".join(((k + challenge(i, bb, rec) * s) % R).to_bytes(32, "little") for i, (s, k) in enumerate(zip(secrets, nonces)))


def record_points(rec):
    """(A, T): three points each"""
    return [g1_at(rec, REC_A + 8 * s) for s in range(3)], [g1_at(rec, REC_T + 8 * s) for s in range(3)]


def knowledge_failed(before, rec):
    """bit s set where z_s·B_s != T_s + c_s·A_s"""
    A, T = record_points(rec)
    bb, failed = points_bytes(before), 0
    for s in range(3):
        z = coord(rec, REC_Z + 4 * s)
        if z >= R or bp.g1_mul(dec1(before[s]), z) != bp.g1_add(dec1(T[s]), bp.g1_mul(dec1(A[s]), challenge(s, bb, rec))):
            failed |= 1 << s
    return failed


# ---- the verdict ---------------------------------------------------------------------------------------------------------------------------------------
def point_bits(p):
    if max(p) >= Q:
        return COORD
    if dec1(p) is None:
        return IDENTITY
    return 0 if bp.g1_on_curve(p) else OFF_CURVE


@functools.lru_cache(maxsize=None)
def _judge(frozen, rho):
    return V.judge({name: list(pts) for name, pts in frozen}, list(rho))


def split_records(records):
    if len(records) % RECORD_BYTES:
        raise ValueError("records are 488 bytes each")
    recs = [records[k:k + RECORD_BYTES] for k in range(0, len(records), RECORD_BYTES)]
    for j, r in enumerate(recs):
        if int.from_bytes(r[:8], "little") != RECORD_MAGIC:
            raise ValueError(f"record {j} is not a contribution record")
    return recs


def verify(origin, final, records, rho=None):
    """(bits, string_bits, (what, index)) of a chain: origin = three points, final = a string of points, records = bytes; rho: the scalars of the string's combinations
    (default: fixed_rho).  ValueError for what the library answers VIMZ_ERR_INVALID to."""
    recs = split_records(records)
    for s, p in enumerate(origin):
        if point_bits(p):
            return point_bits(p), 0, (AT_ORIGIN, s)
    for j, r in enumerate(recs):
        A, T = record_points(r)
        b = 0
        for p in A + T:
            b |= point_bits(p)
        if b:
            return b, 0, (AT_RECORD, j)
    bits, first, before = 0, (0, 0), list(origin)
    for j, r in enumerate(recs):
        failed = knowledge_failed(before, r)
        if failed and not bits:
            first = (AT_RECORD, j)
        for s in range(3):
            if failed >> s & 1:
                bits |= KNOWLEDGE[s]
        before = record_points(r)[0]
    if [tuple(p) for p in before] != [tuple(p) for p in base_points(final)]:
        bits |= LAST
    if bits:
        return bits, 0, first
    if rho is None:
        rho = fixed_rho(len(final["tau_g1"]) - 1)
    sbits, sfirst = _judge(tuple((name, tuple(final[name])) for name in V.ARRAYS[1:]), tuple(rho))
    if sbits:
        return STRING, sbits, ((AT_RECORD + sfirst[0], sfirst[1]) if sfirst[0] else (0, 0))
    return 0, 0, (0, 0)


def fixed_rho(n, label="rho"):
    rng = random.Random(f"powers_contrib/{label}/{n}")
    return [rng.getrandbits(128) for _ in range(n)]


# ---- chains on scalars: the strings the tests run ------------------------------------------------------------------------------------------------------------
TAU0, ALPHA0, BETA0 = 0x2545F4914F6CDD1D0123456789ABCDEF % R, 0xFEDCBA987654321, 0x55AA55AA55AA77
SECRET_SETS = ((0x1B2C3D4E5F60718293A4B5C6D7E8F9010203040506070809 % R, 0x9E3779B97F4A7C15F39CC0605CEDC835, R - 2),
               (0xFEDCBA98765432100F1E2D3C4B5A6978, 3, 0x0123456789ABCDEFFEDCBA9876543210AABBCCDDEEFF0011 % R),
               (R - 1, 0x55AA55AA55AA77, 0x1111111122222222333333334444444455555555))      # (tau', alpha', beta') of contributors 0, 1, 2
NONCE_SETS = ((0x0123456789ABCDEFFEDCBA98765432100A0B0C0D0E0F1011, 0x77, R - 5), (5, 0x1F3D5B79A1C3E5F7092B4D6F81A3C5E7, 9), (11, 13, 0xDEADBEEFDEADBEEFDEADBEEF))
OTHER_SECRETS, OTHER_NONCES = (0xABCDEF, 0x123457, 0x765431), (21, 22, 23)      # "the last record of another string"
POWERS = (1, 2, 3, 7)                                          # the strings of the API tests: tau_g1 of 3, 7, 15, 255 points
TAMPER_POWER = 2


@functools.lru_cache(maxsize=None)
def chain_scalars(power, n_records=3, new=False):
    """[string of scalars after 0, 1, .. n_records contributions] from the string of (TAU0, ALPHA0, BETA0) — or, new: of (1, 1, 1), iden3.new_powers' string"""
    strings = [P.string_scalars(*((1, 1, 1) if new else (TAU0, ALPHA0, BETA0)), power)]
    for j in range(n_records):
        strings.append(contribute_scalars(strings[-1], *SECRET_SETS[j]))
    return strings


def triple(s):
    """(tau, alpha, beta) of a string of scalars"""
    return s["tau_g1"][1], s["alpha_g1"][0], s["beta_g1"][0]


def scalar_points(triple_):
    return [V.mul(1, x) for x in triple_]


@functools.lru_cache(maxsize=None)
def chain_records(n_records=3, new=False):
    """the records of chain_scalars' contributions, one after another (they depend on the string's three points alone, not on its power)"""
    strings = chain_scalars(1, n_records, new)
    return b"".join(make_record(scalar_points(triple(strings[j])), SECRET_SETS[j], NONCE_SETS[j]) for j in range(n_records))


@functools.lru_cache(maxsize=None)
def chain(power=TAMPER_POWER, n_records=3):
    """(origin points, final string of points, records)"""
    strings = chain_scalars(power, n_records)
    return scalar_points(triple(strings[0])), V.string_points(strings[-1]), chain_records(n_records)


# ---- tampered chains -----------------------------------------------------------------------------------------------------------------------------------
def tamper_table():
    """name -> (bits, string_bits, first_bad) of the three-record chain at TAMPER_POWER with ONE thing wrong each (tampered_chains makes them).  The bits follow from
    the stages and from what each challenge hashes (the three B, the three A and the secret's own T): a changed A spoils the three proofs of its record AND, as the
    base of the next record, that record's three; a changed T or z spoils the one proof; swapped, dropped-in-the-middle or foreign records are proofs over bases
    they were not made for.  No curve arithmetic here: cheap enough for a test's parameters."""
    table = {}
    for s, name in enumerate(SECRETS):
        table[f"record_A/{name}"] = (KNOWLEDGE_ALL, 0, (AT_RECORD, 1))
        table[f"record_T/{name}"] = (KNOWLEDGE[s], 0, (AT_RECORD, 1))
        table[f"record_z/{name}"] = (KNOWLEDGE[s], 0, (AT_RECORD, 1))
    table.update({"records_swapped": (KNOWLEDGE_ALL, 0, (AT_RECORD, 0)), "last_record_dropped": (LAST, 0, (0, 0)), "middle_record_dropped": (KNOWLEDGE_ALL, 0, (AT_RECORD, 1)),
                  "last_record_of_another_string": (KNOWLEDGE_ALL | LAST, 0, (AT_RECORD, 2)),
                  "final_point/tau_g1": (STRING, V.RATIO_TAU_G1, (0, 0)), "final_point/tau_g2": (STRING, V.RATIO_TAU_G2, (0, 0)), "final_point/alpha_g1": (STRING, V.RATIO_ALPHA_G1, (0, 0)),
                  "final_point/beta_g1": (STRING, V.RATIO_BETA_G1, (0, 0)), "final_point/beta_g2": (STRING, V.BETA, (0, 0)),
                  "final_point_off_curve": (STRING, V.OFF_CURVE, (AT_RECORD + 1, 3)),
                  "record_point_identity": (IDENTITY, 0, (AT_RECORD, 1)), "record_point_off_curve": (OFF_CURVE, 0, (AT_RECORD, 1)), "origin_coordinate_is_q": (COORD, 0, (AT_ORIGIN, 0))})
    return table


@functools.lru_cache(maxsize=None)
def tampered_chains():
    """name -> (origin, final, records) for every name of tamper_table"""
    origin, final, records = chain()
    rec = split_records(records)
    join = lambda *r: b"".join(r)      # noqa: E731
    seven = lambda p: bp.g1_mul(p, 7)      # noqa: E731
    cases = {}
    for s, name in enumerate(SECRETS):
        A, T = record_points(rec[1])
        cases[f"record_A/{name}"] = (origin, final, join(rec[0], put(rec[1], REC_A + 8 * s, g1_bytes(seven(A[s]))), rec[2]))
        cases[f"record_T/{name}"] = (origin, final, join(rec[0], put(rec[1], REC_T + 8 * s, g1_bytes(seven(T[s]))), rec[2]))
        cases[f"record_z/{name}"] = (origin, final, join(rec[0], put(rec[1], REC_Z + 4 * s, ((coord(rec[1], REC_Z + 4 * s) + 1) % R).to_bytes(32, "little")), rec[2]))
    cases["records_swapped"] = (origin, final, join(rec[1], rec[0], rec[2]))
    cases["last_record_dropped"] = (origin, final, join(rec[0], rec[1]))
    cases["middle_record_dropped"] = (origin, final, join(rec[0], rec[2]))
    other = make_record(scalar_points((12345, 678, 91011)), OTHER_SECRETS, OTHER_NONCES)
    cases["last_record_of_another_string"] = (origin, final, join(rec[0], rec[1], other))

    def with_point(name, k, p):
        out = dict(final)
        out[name] = list(final[name])
        out[name][k] = p
        return out
    for name in ("tau_g1", "alpha_g1", "beta_g1"):
        k = 3 if name == "tau_g1" else 2
        cases[f"final_point/{name}"] = (origin, with_point(name, k, seven(final[name][k])), records)
    cases["final_point/tau_g2"] = (origin, with_point("tau_g2", 2, bp.g2_mul(final["tau_g2"][2], 7)), records)
    cases["final_point/beta_g2"] = (origin, with_point("beta_g2", 0, bp.g2_mul(final["beta_g2"][0], 7)), records)
    p = final["tau_g1"][3]
    cases["final_point_off_curve"] = (origin, with_point("tau_g1", 3, (p[0], (p[1] + 1) % Q)), records)
    A, T = record_points(rec[1])
    cases["record_point_identity"] = (origin, final, join(rec[0], put(rec[1], REC_A + 8, bytes(64)), rec[2]))
    cases["record_point_off_curve"] = (origin, final, join(rec[0], put(rec[1], REC_T + 16, g1_bytes((T[2][0], (T[2][1] + 1) % Q))), rec[2]))
    cases["origin_coordinate_is_q"] = ([(Q, origin[0][1])] + origin[1:], final, records)
    assert set(cases) == set(tamper_table())
    return cases


REFUSED_STRINGS = {"coordinate_is_q": "a coordinate is not below q", "tau_g2_off_curve": "a point is not on its curve", "alpha_g1_off_curve": "a point is not on its curve",
                   "tau_g1_1_identity": "tau_g1[1], alpha_g1[0] or beta_g1[0] is the identity", "beta_g1_0_identity": "tau_g1[1], alpha_g1[0] or beta_g1[0] is the identity"}


def refused_strings():
    """name -> a string of points vimz_powers_contribute refuses with REFUSED_STRINGS' message"""
    s = V.string_points(chain_scalars(TAMPER_POWER, 0)[0])

    def with_point(name, k, p):
        out = dict(s)
        out[name] = list(s[name])
        out[name][k] = p
        return out
    t2, a = s["tau_g2"][2], s["alpha_g1"][1]
    return {"coordinate_is_q": with_point("beta_g1", 3, (s["beta_g1"][3][0], Q)), "tau_g2_off_curve": with_point("tau_g2", 2, (t2[0], ((t2[1][0] + 1) % Q, t2[1][1]))),
            "alpha_g1_off_curve": with_point("alpha_g1", 1, (a[0], (a[1] + 1) % Q)), "tau_g1_1_identity": with_point("tau_g1", 1, V.G1_ZERO),
            "beta_g1_0_identity": with_point("beta_g1", 0, V.G1_ZERO)}


# ---- the cases of the two kernels, on SCALARS ---------------------------------------------------------------------------------------------------------------
POWER_COUNTS = (1, 2, 3, 63, 64, 65, 129, 1025)                # bit counts 0, 1, 2, 6, 6, 7, 8, 11: half a block, a full block, ragged blocks
W_RANDOM = (0x2F1E0D3C4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1 % R) | (1 << 250)
C_RANDOM = 0x1D4B8E2A6F9C3071B5E8D2A4C6F80913579BDF02468ACE13579BDF0246801357 % R
assert (1 << 250) <= W_RANDOM < R
POWER_WS = {"one": 1, "r_minus_1": R - 1, "two": 2, "random": W_RANDOM}
SCALE_N = {1: (1, 63, 64, 65, 129), 2: (1, 63, 64, 65)}
BASE_D = 0x1F3D5B79A1C3E5F7092B4D6F81A3C5E7 % R


def bitlen_of_count(count):
    """the trip count the host hands k_power_vec"""
    return (count - 1).bit_length()


def scale_inputs(n):
    """the scalars of the n input points: an identity at index 0 and at n/2 (the same slot when n = 1)"""
    s = [BASE_D * (5 + 3 * k) % R for k in range(n)]
    s[0] = s[n // 2] = 0
    return s


def scale_cases(group):
    """name -> (input scalars, w, c, form, in_place) per size: c = 1 and c random; w = 1 with c = 1 (the output is the input); w = r − 1 (the scalars alternate between
    1 and the full 254-bit walk of r − 1); w random; c = 0 (every output the identity; the hook alone passes it); in place; the Montgomery form"""
    cases = {}
    for n in SCALE_N[group]:
        s = scale_inputs(n)
        cases[f"{n}/w_one_c_one"] = (s, 1, 1, "canonical", False)
        cases[f"{n}/w_r_minus_1"] = (s, R - 1, 1, "canonical", False)
        cases[f"{n}/w_random_c_one"] = (s, W_RANDOM, 1, "canonical", False)
        cases[f"{n}/w_random_c_random"] = (s, W_RANDOM, C_RANDOM, "canonical", False)
        cases[f"{n}/c_zero"] = (s, W_RANDOM, 0, "canonical", False)
        cases[f"{n}/in_place"] = (s, W_RANDOM, C_RANDOM, "canonical", True)
        cases[f"{n}/montgomery"] = (s, 2, C_RANDOM, "montgomery", True)
    return cases


def scale_expected(s, w, c):
    return [x * c * pow(w, k, R) % R for k, x in enumerate(s)]
