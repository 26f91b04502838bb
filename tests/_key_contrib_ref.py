"""Further delta contributions to a saved decider key (vimz_decider_key_contribute / vimz_decider_key_verify_contributions; vimz_amd/csrc/g16_key_contrib.hip and
.hpp) stated in plain Python integers on tests/_pairing.py's arithmetic: the blob's parser, contribute, the record and its challenge, the whole verdict — and the
synthetic keys and tampered chains the CPU tests (tests/test_key_contrib_ref_host.py) and the GPU tests (tests/test_gpu_key_contrib.py) run.  A key is bytes in
vimz_decider_key_save's layout; the synthetic ones hold points [s]G of known scalars and belong to no circuit: the layout is read from the header.  No GPU, no numpy.
Test infrastructure."""
import functools
import hashlib
import secrets

from tests import _pairing as bp
from tests._pairing import Q, R
from tests._powers_verify_ref import g2_mul_raw

KEY_MAGIC, RECORD_MAGIC = int.from_bytes(b"VG16KEY2", "little"), int.from_bytes(b"VG16CTR1", "little")
RECORD_WORDS, RECORD_BYTES = 37, 296
KEY_HEAD_WORDS, KEY_DELTA1, KEY_DELTA2, KEY_IC = 11, 43, 83, 99      # word offsets of a key blob (g16_key_contrib.hpp)
REC_DELTA1, REC_DELTA2, REC_T, REC_Z = 1, 9, 25, 33                  # ... of a record
TAG = b"vimz-decider-key-contribution"
COORD, OFF_CURVE, IDENTITY, SUBGROUP, FIXED_PART, DELTA_HALVES, KNOWLEDGE, LAST, RATIO = (1 << k for k in range(9))      # VIMZ_KEYCHAIN_*
AT_ORIGIN_DELTA, AT_FINAL_DELTA, AT_RECORD, AT_ORIGIN_LH, AT_FINAL_LH, AT_FIXED_PART = range(1, 7)                      # VIMZ_KEYCHAIN_AT_*
RLC_CHUNK, PT_BLOCK = 8, 64


# ---- bytes <-> points (canonical little-endian coordinates; the identity as zeros) ------------------------------------------------------------------
def coord(blob, word):
    return int.from_bytes(blob[8 * word:8 * word + 32], "little")


def g1_at(blob, word):
    return coord(blob, word), coord(blob, word + 4)


def g2_at(blob, word):
    return (coord(blob, word), coord(blob, word + 4)), (coord(blob, word + 8), coord(blob, word + 12))


def g1_bytes(p):
    x, y = (0, 0) if p is None else p
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def g2_bytes(p):
    (x0, x1), (y0, y1) = ((0, 0), (0, 0)) if p is None else p
    return b"".join(c.to_bytes(32, "little") for c in (x0, x1, y0, y1))


def dec1(p):
    return None if p == (0, 0) else p


def dec2(p):
    return None if p == ((0, 0), (0, 0)) else p


def put(blob, word, data):
    return blob[:8 * word] + data + blob[8 * word + len(data):]


# ---- the blob's layout, from its own header ----------------------------------------------------------------------------------------------------------
def layout(blob):
    """{"words", "off_lh", "n_lh", "m", "n_pub", "n"} or ValueError with the library's message"""
    if len(blob) % 8 or len(blob) // 8 < KEY_IC:
        raise ValueError("not a decider key")
    w = [int.from_bytes(blob[8 * k:8 * k + 8], "little") for k in range(7)]
    m, n_pub, n = w[1], w[2], w[4]
    if w[0] != KEY_MAGIC or w[6] > 1 or m >= 1 << 31 or n >= 1 << 31 or not n or n_pub >= m:
        raise ValueError("not a decider key")
    n_l, n_h = m - n_pub - 1, n - 1
    words = KEY_IC + 8 * (n_pub + 1) + 8 * (2 * m + n_l + n_h) + 16 * m
    if words != len(blob) // 8:
        raise ValueError("wrong length")
    return {"words": words, "off_lh": KEY_IC + 8 * (n_pub + 1) + 16 * m, "n_lh": n_l + n_h, "m": m, "n_pub": n_pub, "n": n}


def lh_points(blob):
    L = layout(blob)
    return [g1_at(blob, L["off_lh"] + 8 * i) for i in range(L["n_lh"])]


# ---- the record ----------------------------------------------------------------------------------------------------------------------------------------
def challenge(head, delta1_before, record):
    """c of a record: head = the key's first 88 bytes, delta1_before 64 bytes; SHA3-256 read as groth16.hip's fr_from_hash reads a digest (the top byte cleared)"""
    d = hashlib.sha3_256(TAG + head + delta1_before + record[8 * REC_DELTA1:8 * REC_Z]).digest()
    return int.from_bytes(d[:31], "little")


def make_record(head, delta1, delta2, delta, nonce):
    """(record, delta1 after, delta2 after) for the points delta1, delta2 before"""
    after1, after2, T = bp.g1_mul(delta1, delta), bp.g2_mul(delta2, delta), bp.g1_mul(delta1, nonce)
    rec = RECORD_MAGIC.to_bytes(8, "little") + g1_bytes(after1) + g2_bytes(after2) + g1_bytes(T)
    z = (nonce + challenge(head, g1_bytes(delta1), rec) * delta) % R
    return rec + z.to_bytes(32, "little"), after1, after2


def contribute(blob, delta, nonce):
    """(key of delta·delta', record), or ValueError with vimz_decider_key_contribute's message"""
    L = layout(blob)
    d1, d2 = g1_at(blob, KEY_DELTA1), g2_at(blob, KEY_DELTA2)
    pts = lh_points(blob)
    if max(d1 + d2[0] + d2[1]) >= Q or any(max(p) >= Q for p in pts):
        raise ValueError("a coordinate is not below q")
    if not bp.g1_on_curve(dec1(d1)) or not bp.g2_on_curve(dec2(d2)):
        raise ValueError("a delta point is not on its curve")
    if dec1(d1) is None or dec2(d2) is None:
        raise ValueError("a delta point is the identity")
    if g2_mul_raw(d2, R) is not None:
        raise ValueError("delta2 is outside the subgroup")
    assert 0 < delta < R and 0 <= nonce < R
    rec, a1, a2 = make_record(blob[:8 * KEY_HEAD_WORDS], d1, d2, delta, nonce)
    dinv = pow(delta, -1, R)
    out = put(put(blob, KEY_DELTA1, g1_bytes(a1)), KEY_DELTA2, g2_bytes(a2))
    out = put(out, L["off_lh"], b"".join(g1_bytes(bp.g1_mul(dec1(p), dinv)) for p in pts))
    return out, rec


# ---- the verdict ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _product_is_one(pairs):
    return bp.pairing_product_is_one(list(pairs))


def g1_bits(p, may_be_identity=False):
    if max(p) >= Q:
        return COORD
    if dec1(p) is None:
        return 0 if may_be_identity else IDENTITY
    return 0 if bp.g1_on_curve(p) else OFF_CURVE


@functools.lru_cache(maxsize=None)
def g2_bits(p):
    if max(p[0] + p[1]) >= Q:
        return COORD
    if dec2(p) is None:
        return IDENTITY
    if not bp.g2_on_curve(p):
        return OFF_CURVE
    return SUBGROUP if g2_mul_raw(p, R) is not None else 0


def knowledge_holds(head, delta1_before, rec):
    z = coord(rec, REC_Z)
    if z >= R:
        return False
    c = challenge(head, g1_bytes(delta1_before), rec)
    return bp.g1_mul(dec1(delta1_before), z) == bp.g1_add(dec1(g1_at(rec, REC_T)), bp.g1_mul(g1_at(rec, REC_DELTA1), c))


def verify(origin, final, records, rho=None):
    """(bits, (what, index)) of a chain — records: bytes, RECORD_BYTES each —, or ValueError for what the library answers VIMZ_ERR_INVALID to.  rho: the n_lh scalars
    of the same-ratio check (default: 128 bits each from the OS)"""
    Lo, Lf = layout(origin), layout(final)
    if len(records) % RECORD_BYTES:
        raise ValueError("records are 296 bytes each")
    recs = [records[k:k + RECORD_BYTES] for k in range(0, len(records), RECORD_BYTES)]
    for j, r in enumerate(recs):
        if int.from_bytes(r[:8], "little") != RECORD_MAGIC:
            raise ValueError(f"record {j} is not a contribution record")
    if Lo["words"] != Lf["words"] or origin[:56] != final[:56]:
        return FIXED_PART, (AT_FIXED_PART, next((k for k in range(7) if origin[8 * k:8 * k + 8] != final[8 * k:8 * k + 8]), 7))
    n = Lo["n_lh"]
    # the points
    for blob, what in ((origin, AT_ORIGIN_DELTA), (final, AT_FINAL_DELTA)):
        b1, b2 = g1_bits(g1_at(blob, KEY_DELTA1)), g2_bits(g2_at(blob, KEY_DELTA2))
        if b1 | b2:
            return b1 | b2, (what, 0 if b1 else 1)
    for j, r in enumerate(recs):
        b = g1_bits(g1_at(r, REC_DELTA1)) | g2_bits(g2_at(r, REC_DELTA2)) | g1_bits(g1_at(r, REC_T), may_be_identity=True)
        if b:
            return b, (AT_RECORD, j)
    P = (lh_points(origin), lh_points(final))

    def flag(side, i):
        p, o = P[side][i], P[1 - side][i]
        if max(p) >= Q:
            return COORD
        if dec1(p) is None:
            return 0 if max(o) >= Q or dec1(o) is None else IDENTITY
        return 0 if bp.g1_on_curve(p) else OFF_CURVE
    for side, what in ((0, AT_ORIGIN_LH), (1, AT_FINAL_LH)):
        f = [flag(side, i) for i in range(n)]
        if any(f):
            bits = 0
            for x in f:
                bits |= x
            return bits, (what, next(i for i, x in enumerate(f) if x))
    # the fixed part
    skip = set(range(KEY_DELTA1, KEY_DELTA1 + 8)) | set(range(KEY_DELTA2, KEY_DELTA2 + 16)) | set(range(Lo["off_lh"], Lo["off_lh"] + 8 * n))
    for k in range(Lo["words"]):
        if k not in skip and origin[8 * k:8 * k + 8] != final[8 * k:8 * k + 8]:
            return FIXED_PART, (AT_FIXED_PART, k)
    # the equations, all of them
    head = origin[:8 * KEY_HEAD_WORDS]
    bits, first = 0, (0, 0)
    before = g1_at(origin, KEY_DELTA1)
    for j, r in enumerate(recs):
        d1, d2 = g1_at(r, REC_DELTA1), g2_at(r, REC_DELTA2)
        b = 0 if _product_is_one(((d1, bp.G2), (bp.g1_neg(bp.G1), d2))) else DELTA_HALVES
        if not knowledge_holds(head, before, r):
            b |= KNOWLEDGE
        if b and not bits:
            first = (AT_RECORD, j)
        bits |= b
        before = d1
    last1, last2 = (recs[-1][8 * REC_DELTA1:8 * REC_DELTA2], recs[-1][8 * REC_DELTA2:8 * REC_T]) if recs else (origin[8 * KEY_DELTA1:8 * KEY_DELTA1 + 64], origin[8 * KEY_DELTA2:8 * KEY_DELTA2 + 128])
    if last1 != final[8 * KEY_DELTA1:8 * KEY_DELTA1 + 64] or last2 != final[8 * KEY_DELTA2:8 * KEY_DELTA2 + 128]:
        bits |= LAST
    if rho is None:
        rho = [secrets.randbits(128) for _ in range(n)]
    S, S1 = ratio_sums(P[0], P[1], rho)
    if not _product_is_one(((S1, g2_at(final, KEY_DELTA2)), (bp.g1_neg(S), g2_at(origin, KEY_DELTA2)))):
        bits |= RATIO
    return bits, first


def fixed_rho(n, label="rho"):
    """n scalars of 128 bits from a seed: what a test passes for rho so that equal chains meet equal pairings (the library draws its own from the OS)"""
    import random
    rng = random.Random(f"key_contrib/{label}/{n}")
    return [rng.getrandbits(128) for _ in range(n)]


def ratio_sums(before, after, rho):
    """S = Σ rho_i·before_i, S' = Σ rho_i·after_i on points (raw pairs, the identity as zeros)"""
    S = S1 = None
    for p, q, k in zip(before, after, rho):
        S, S1 = bp.g1_add(S, bp.g1_mul(dec1(p), k)), bp.g1_add(S1, bp.g1_mul(dec1(q), k))
    return S, S1


# ---- synthetic keys -----------------------------------------------------------------------------------------------------------------------------------
DELTA0 = 0x1B2C3D4E5F60718293A4B5C6D7E8F9010203040506070809 % R
DELTAS = (0x2545F4914F6CDD1D0123456789ABCDEF0011223344556677, 0xFEDCBA98765432100F1E2D3C4B5A6978, 0x55AA55AA55AA77)      # the contributors' delta'
NONCES = (0x0123456789ABCDEFFEDCBA98765432100A0B0C0D0E0F1011, 0x1111111122222222333333334444444455555555, 0x77)
SMALL, LARGE = (6, 1, 4), (14, 1, 8)      # (m, n_pub, n): l‖h of 7 points (one chunk of the combination) and of 19 (three chunks)


@functools.lru_cache(maxsize=None)
def synthetic_key(delta, shape=SMALL, identity_in_l=None):
    """a key blob of that shape whose points are [s]G: delta1 = [delta]G1, delta2 = [delta]G2, l‖h_i = [u_i / delta]G1 with u_i fixed — so the key of delta·delta' IS the
    key of delta after a contribution of delta' —, everything else small multiples.  identity_in_l: an index of l‖h whose point is the identity."""
    m, n_pub, n = shape
    n_lh = (m - n_pub - 1) + (n - 1)
    g1 = lambda s: g1_bytes(bp.g1_mul(bp.G1, s))      # noqa: E731
    g2 = lambda s: g2_bytes(bp.g2_mul(bp.G2, s))      # noqa: E731
    dinv = pow(delta, -1, R)
    head = b"".join(x.to_bytes(8, "little") for x in (KEY_MAGIC, m, n_pub, n - n_pub - 1, n, 1, 1)) + (0x0123456789ABCDEF ** 3 % R).to_bytes(32, "little")
    parts = [head, g2(11), g1(12), g1(13), g1(delta), g2(13), g2(1), g2(delta)]
    parts += [g1(100 + i) for i in range(n_pub + 1)]
    parts += [g1(200 + i) for i in range(m)] + [g1(300 + i) for i in range(m)]
    parts += [b"\0" * 64 if i == identity_in_l else g1((0x9E3779B97F4A7C15F39CC0605CEDC835 * (i + 1) % R) * dinv % R) for i in range(n_lh)]
    parts += [b"\0" * 128 if i % 3 == 2 else g2(400 + i) for i in range(m)]
    blob = b"".join(parts)
    assert layout(blob)["n_lh"] == n_lh
    return blob


@functools.lru_cache(maxsize=None)
def chain(shape=SMALL, n_records=3, identity_in_l=None):
    """(origin, final, records) of n_records contributions DELTAS[j] with NONCES[j] on the synthetic key of DELTA0"""
    origin = key = synthetic_key(DELTA0, shape, identity_in_l)
    records = b""
    for j in range(n_records):
        key, rec = contribute(key, DELTAS[j], NONCES[j])
        records += rec
    return origin, key, records


def tamper_table(shape=SMALL):
    """name -> (bits, first_bad) of the three-record chain with ONE thing wrong each (tampered_chains makes them); the bits follow from the verdict's stages and
    equations (include/vimz_hip.h).  A delta2 replaced in a record also changes that record's challenge, so its proof of knowledge fails with it; swapping records
    0 and 1 breaks every proof of knowledge (each was made over another base) and nothing else.  No curve arithmetic here: cheap enough for a test's parameters."""
    m, n_pub, n = shape
    n_lh = (m - n_pub - 1) + (n - 1)
    table = {f"l_h_point_scaled/{name}": (RATIO, (0, 0)) for name in ("first", "last") + (("second_chunk",) if n_lh > RLC_CHUNK + 1 else ())}
    table.update({"h_points_swapped": (RATIO, (0, 0)), "l_point_off_curve": (OFF_CURVE, (AT_FINAL_LH, 2)), "coordinate_is_q": (COORD, (AT_FINAL_LH, 3)),
                  "identity_in_one_key": (IDENTITY, (AT_FINAL_LH, 5)), "a_query_byte": (FIXED_PART, (AT_FIXED_PART, KEY_IC + 8 * (n_pub + 1) + 8 * 2 + 1)),
                  "record_delta2_replaced": (DELTA_HALVES | KNOWLEDGE, (AT_RECORD, 1)), "record_z_off_by_one": (KNOWLEDGE, (AT_RECORD, 1)),
                  "records_swapped": (KNOWLEDGE, (AT_RECORD, 0)), "last_record_dropped": (LAST, (0, 0))})
    return table


def tampered_chains(shape=SMALL):
    """name -> (origin, final, records) for every name of tamper_table"""
    origin, final, records = chain(shape, 3)
    L = layout(final)
    n, off = L["n_lh"], L["off_lh"]
    n_l = L["m"] - L["n_pub"] - 1
    rec = [records[k:k + RECORD_BYTES] for k in range(0, len(records), RECORD_BYTES)]
    pt = lambda i: g1_at(final, off + 8 * i)      # noqa: E731
    cases = {}
    for name, i in [("first", 0), ("last", n - 1)] + ([("second_chunk", RLC_CHUNK + 1)] if n > RLC_CHUNK + 1 else []):
        cases[f"l_h_point_scaled/{name}"] = (origin, put(final, off + 8 * i, g1_bytes(bp.g1_mul(pt(i), 7))), records)
    cases["h_points_swapped"] = (origin, put(put(final, off + 8 * n_l, g1_bytes(pt(n_l + 1))), off + 8 * (n_l + 1), g1_bytes(pt(n_l))), records)
    cases["l_point_off_curve"] = (origin, put(final, off + 8 * 2, g1_bytes((pt(2)[0], (pt(2)[1] + 1) % Q))), records)
    cases["coordinate_is_q"] = (origin, put(final, off + 8 * 3, g1_bytes((Q, pt(3)[1]))), records)
    cases["identity_in_one_key"] = (origin, put(final, off + 8 * 5, b"\0" * 64), records)
    a_word = tamper_table(shape)["a_query_byte"][1][1]      # inside the a query's third point
    cases["a_query_byte"] = (origin, put(final, a_word, bytes([final[8 * a_word] ^ 1])), records)
    cases["record_delta2_replaced"] = (origin, final, rec[0] + put(rec[1], REC_DELTA2, g2_bytes(bp.g2_mul(bp.G2, 0xABCDEF))) + rec[2])
    cases["record_z_off_by_one"] = (origin, final, rec[0] + put(rec[1], REC_Z, ((coord(rec[1], REC_Z) + 1) % R).to_bytes(32, "little")) + rec[2])
    cases["records_swapped"] = (origin, final, rec[1] + rec[0] + rec[2])
    cases["last_record_dropped"] = (origin, final, rec[0] + rec[1])
    assert set(cases) == set(tamper_table(shape))
    return cases


REFUSED_KEYS = ("delta1_coordinate_is_q", "delta1_off_curve", "delta2_identity", "l_coordinate_is_q", "odd_length", "oversized", "short", "truncated", "wrong_magic")


def refused_keys(shape=SMALL):
    """name -> (blob, the message vimz_decider_key_contribute refuses it with)"""
    key = synthetic_key(DELTA0, shape)
    off = layout(key)["off_lh"]
    d1 = g1_at(key, KEY_DELTA1)
    return {"wrong_magic": (put(key, 0, b"VG16KEY1"), "not a decider key"), "truncated": (key[:-8], "wrong length"), "oversized": (key + b"\0" * 8, "wrong length"),
            "short": (key[:64], "not a decider key"), "odd_length": (key[:-3], "not a decider key"),
            "delta1_coordinate_is_q": (put(key, KEY_DELTA1, g1_bytes((Q, d1[1]))), "a coordinate is not below q"),
            "l_coordinate_is_q": (put(key, off + 8, g1_bytes((1, Q))), "a coordinate is not below q"),
            "delta1_off_curve": (put(key, KEY_DELTA1, g1_bytes((d1[0], (d1[1] + 1) % Q))), "a delta point is not on its curve"),
            "delta2_identity": (put(key, KEY_DELTA2, b"\0" * 128), "a delta point is the identity")}


# ---- the cases of the combination (k_ratio_rlc through vimz_test_ratio_rlc), on SCALARS: a point [s]G is its s ------------------------------------------------
RATIO_SIZES = (1, RLC_CHUNK - 1, RLC_CHUNK, RLC_CHUNK + 1, 19, PT_BLOCK * RLC_CHUNK, PT_BLOCK * RLC_CHUNK + 1, 1030)
MAX128 = (1 << 128) - 1
BASE_D = 0x1F3D5B79A1C3E5F7092B4D6F81A3C5E7 % R


def ratio_cases():
    """name -> (before scalars, after scalars, rho).  Per size: `multiple` — after = 5·before, with an identity at the same index of both, a zero rho, an all-ones rho,
    equal neighbours with equal rho (add_mixed's doubling) and, from two chunks on, a second chunk of two opposite points with equal rho that cancels to the
    identity —; `unrelated` — after is another progression: the kernel sums, it does not judge.  `whole_sum_identity`: two points, opposite, equal rho, in both arrays."""
    import random
    cases = {}
    for n in RATIO_SIZES:
        rng = random.Random(f"ratio/{n}")
        before = [BASE_D * (3 + k) % R for k in range(n)]
        rho = [rng.getrandbits(128) for _ in range(n)]
        if n >= RLC_CHUNK - 1:
            before[2] = 0                                          # an identity (the same index of both arrays)
            rho[3], rho[4] = 0, MAX128
            before[6], rho[6], rho[5] = before[5], rho[5], rho[5]  # equal neighbours, equal rho
        if n >= 2 * RLC_CHUNK:
            before[RLC_CHUNK:2 * RLC_CHUNK] = [0] * RLC_CHUNK      # chunk 1: two opposite points with one rho, identities otherwise
            before[RLC_CHUNK], before[RLC_CHUNK + 1], rho[RLC_CHUNK + 1] = BASE_D, R - BASE_D, rho[RLC_CHUNK]
        cases[f"{n}/multiple"] = (before, [5 * s % R for s in before], rho)
        cases[f"{n}/unrelated"] = (before, [(BASE_D + 12345) * (7 + 2 * k) % R if s else 0 for k, s in enumerate(before)], rho)
    cases["2/whole_sum_identity"] = ([BASE_D, R - BASE_D], [5 * BASE_D % R, R - 5 * BASE_D % R], [0xDEADBEEF << 64 | 1] * 2)
    return cases


def ratio_scalars(before, after, rho):
    return sum(k * s for k, s in zip(rho, before)) % R, sum(k * s for k, s in zip(rho, after)) % R


def ratio_chunk_scalars(s, rho):
    return [sum(rho[i] * s[i] for i in range(lo, min(lo + RLC_CHUNK, len(s)))) % R for lo in range(0, len(s), RLC_CHUNK)]
