"""Packed curve points and packed decider keys (vimz_points_pack / _unpack, vimz_decider_key_pack / _unpack; vimz_amd/csrc/g16_point_pack.hpp and .hip) restated in
plain Python integers on tests/_pairing.py's arithmetic: the encoding, both square roots, the per-point findings, the packed key's parser and both directions of
a key — and the points and bad encodings the CPU tests (tests/test_point_pack_ref_host.py, tests/test_point_pack_host.py) and the GPU tests
(tests/test_gpu_point_pack.py) run.  Points are canonical bytes, the identity as zeros, a packed point little-endian with the flags in its top byte.  No GPU, no
numpy.  Test infrastructure."""
import functools
import os
import random
import re

from tests import _pairing as bp
from tests import _key_contrib_ref as kref
from tests._pairing import Q, R

COORD, FLAGS, OFF_CURVE = 1, 2, 4                                # VIMZ_PACK_*
NAMES = {COORD: "coord", FLAGS: "flags", OFF_CURVE: "off_curve"}
INF, SIGN = 1 << 255, 1 << 254                                   # in the 256 bits of x (G1) or of x.c1 (G2)
HALF = (Q - 1) // 2
EXP = (Q + 1) // 4
PACKED_KEY_MAGIC = int.from_bytes(b"VG16KPK1", "little")
KEY_KZG, KEY_ALPHA1, KEY_BETA2, KEY_IC = 11, 27, 51, 99          # word offsets of a key blob's fixed points and first run
PKEY_KZG, PKEY_ALPHA1, PKEY_BETA2, PKEY_IC = 11, 19, 31, 55      # ... of a packed key's
FIXED = ((2, KEY_KZG, PKEY_KZG), (1, KEY_ALPHA1, PKEY_ALPHA1), (1, KEY_ALPHA1 + 8, PKEY_ALPHA1 + 4), (1, KEY_ALPHA1 + 16, PKEY_ALPHA1 + 8),
         (2, KEY_BETA2, PKEY_BETA2), (2, KEY_BETA2 + 16, PKEY_BETA2 + 8), (2, KEY_BETA2 + 32, PKEY_BETA2 + 16))
B1, B2 = 3, bp.B2
assert Q % 4 == 3


def chunk():
    """VIMZ_PACK_CHUNK, from the header that names it"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vimz_hip.h")).read()
    return int(re.search(r"#define VIMZ_PACK_CHUNK (\d+)", text).group(1))


# ---- the square roots -------------------------------------------------------------------------------------------------------------------------------------
def f2_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q


def f2_sqr(a):
    return f2_mul(a, a)


def fq_sqrt(a):
    """a root of a, or None: t = a^((q+1)/4) squares to a or to -a"""
    t = pow(a, EXP, Q)
    return t if t * t % Q == a else None


def fq2_sqrt_candidate(a):
    """the root the algorithm forms, whether or not it is one"""
    a0, a1 = a
    if a1 == 0:
        t = pow(a0, EXP, Q)
        return (t, 0) if t * t % Q == a0 else (0, t)
    s = pow((a0 * a0 + a1 * a1) % Q, EXP, Q)
    d = (a0 + s) * pow(2, -1, Q) % Q
    t = pow(d, EXP, Q)
    w = a1 * pow(2 * t % Q, Q - 2, Q) % Q      # (0 -> 0, as the library's inversion)
    return (t, w) if t * t % Q == d else (w, t)


def fq2_sqrt(a):
    r = fq2_sqrt_candidate(a)
    return r if f2_sqr(r) == a else None


def fq2_is_square(a):
    """the norm criterion: a != 0 is a square in Fq2 iff a0² + a1² is one in Fq (Euler)"""
    n = (a[0] * a[0] + a[1] * a[1]) % Q
    return n == 0 or pow(n, (Q - 1) // 2, Q) == 1


def larger1(y):
    return y > HALF


def larger2(y):
    return y[1] > HALF if y[1] else y[0] > HALF


def rhs1(x):
    return (x * x * x + B1) % Q


def rhs2(x):
    c = f2_mul(f2_sqr(x), x)
    return (c[0] + B2[0]) % Q, (c[1] + B2[1]) % Q


# ---- one point: (value, finding) ----------------------------------------------------------------------------------------------------------------------------
def pack_g1(p):
    """p = (x, y) raw integers below 2^256, the identity (0, 0) -> (the packed 256 bits, 0) or (0, finding)"""
    x, y = p
    if x >= Q or y >= Q:
        return 0, COORD
    if (x, y) == (0, 0):
        return INF, 0
    if y * y % Q != rhs1(x):
        return 0, OFF_CURVE
    return x | (SIGN if larger1(y) else 0), 0


def unpack_g1(v):
    inf, sign, x = v & INF, v & SIGN, v & (SIGN - 1)
    if inf:
        return ((0, 0), 0) if not sign and not x else ((0, 0), FLAGS)
    if x >= Q:
        return (0, 0), COORD
    y = fq_sqrt(rhs1(x))
    if y is None:
        return (0, 0), OFF_CURVE
    if larger1(y) != bool(sign):
        y = Q - y
    return (x, y), 0


def pack_g2(p):
    """p = ((x0, x1), (y0, y1)) -> ((c0 word, c1 word with the flags), 0) or ((0, 0), finding)"""
    x, y = p
    if max(x + y) >= Q:
        return (0, 0), COORD
    if x == (0, 0) and y == (0, 0):
        return (0, INF), 0
    if f2_sqr(y) != rhs2(x):
        return (0, 0), OFF_CURVE
    return (x[0], x[1] | (SIGN if larger2(y) else 0)), 0


def unpack_g2(v):
    zero = ((0, 0), (0, 0))
    f = FLAGS if v[0] >> 254 else 0
    x0 = v[0] & (SIGN - 1)
    inf, sign, x1 = v[1] & INF, v[1] & SIGN, v[1] & (SIGN - 1)
    if inf:
        return zero, (FLAGS if sign or x0 or x1 else f)
    if x0 >= Q or x1 >= Q:
        f |= COORD
    if f:
        return zero, f
    y = fq2_sqrt(rhs2((x0, x1)))
    if y is None:
        return zero, OFF_CURVE
    if larger2(y) != bool(sign):
        y = ((Q - y[0]) % Q, (Q - y[1]) % Q)
    return ((x0, x1), y), 0


# ---- arrays as bytes ------------------------------------------------------------------------------------------------------------------------------------------
def _ints(data, size):
    return [int.from_bytes(data[k:k + 32], "little") for k in range(0, size, 32)]


def pack_point_bytes(group, data):
    """one unpacked point (64 / 128 bytes) -> (32 / 64 packed bytes, finding); zeros with a finding"""
    c = _ints(data, 64 * group)
    if group == 1:
        v, f = pack_g1((c[0], c[1]))
        return v.to_bytes(32, "little"), f
    v, f = pack_g2(((c[0], c[1]), (c[2], c[3])))
    return v[0].to_bytes(32, "little") + v[1].to_bytes(32, "little"), f


def unpack_point_bytes(group, data):
    c = _ints(data, 32 * group)
    if group == 1:
        p, f = unpack_g1(c[0])
        return kref.g1_bytes(p), f
    p, f = unpack_g2((c[0], c[1]))
    return kref.g2_bytes(p), f


@functools.lru_cache(maxsize=None)
def _pack_cached(group, data):
    return pack_point_bytes(group, data)


@functools.lru_cache(maxsize=None)
def _unpack_cached(group, data):
    return unpack_point_bytes(group, data)


def run(group, packing, data):
    """(output bytes or None, bits, first_bad) of vimz_points_pack / _unpack over canonical points: the findings are those of the FIRST point that has one"""
    size = (64 if packing else 32) * group
    assert len(data) % size == 0
    out = []
    for i in range(len(data) // size):
        o, f = (_pack_cached if packing else _unpack_cached)(group, bytes(data[size * i:size * (i + 1)]))
        if f:
            return None, f, i
        out.append(o)
    return b"".join(out), 0, 0


def per_point(group, packing, data):
    """[(slot bytes, finding)] point by point: what every thread leaves"""
    size = (64 if packing else 32) * group
    return [(_pack_cached if packing else _unpack_cached)(group, bytes(data[size * i:size * (i + 1)])) for i in range(len(data) // size)]


MONT = (1 << 256) % Q


def to_form(data, mont):
    """canonical point bytes as they lie in memory in that form: every coordinate below q times 2^256 (one not below q stays: it is refused in either form)"""
    if not mont:
        return data
    return b"".join((c * MONT % Q if c < Q else c).to_bytes(32, "little") for c in _ints(data, len(data)))


def from_form(data, mont):
    if not mont:
        return data
    inv = pow(MONT, -1, Q)
    return b"".join((c * inv % Q).to_bytes(32, "little") for c in _ints(data, len(data)))


# ---- the packed key -------------------------------------------------------------------------------------------------------------------------------------------
def runs(m, n_pub, n):
    n_g1 = (n_pub + 1) + 2 * m + (m - n_pub - 1) + (n - 1)
    return {"n_g1": n_g1, "n_g2": m, "off_g1": KEY_IC, "off_g2": KEY_IC + 8 * n_g1, "words": KEY_IC + 8 * n_g1 + 16 * m,
            "poff_g1": PKEY_IC, "poff_g2": PKEY_IC + 4 * n_g1, "pwords": PKEY_IC + 4 * n_g1 + 8 * m}


def packed_layout(blob):
    """the runs of a packed key, or ValueError with the library's message; every size from the blob's own header"""
    if len(blob) % 8 or len(blob) // 8 < PKEY_IC:
        raise ValueError("not a packed decider key")
    w = [int.from_bytes(blob[8 * k:8 * k + 8], "little") for k in range(7)]
    m, n_pub, n = w[1], w[2], w[4]
    if w[0] != PACKED_KEY_MAGIC or w[6] > 1 or m >= 1 << 31 or n >= 1 << 31 or not n or n_pub >= m:
        raise ValueError("not a packed decider key")
    L = runs(m, n_pub, n)
    if L["pwords"] != len(blob) // 8:
        raise ValueError("wrong length")
    return L


def packed_size(key_bytes):
    """bytes of the packed form of a key of that many bytes: the head, then every point in half"""
    return 88 + (key_bytes - 88) // 2


def _key(blob, packing):
    if packing:
        L0 = kref.layout(blob)
        L = runs(L0["m"], L0["n_pub"], L0["n"])
        assert L["words"] == L0["words"]
    else:
        L = packed_layout(blob)
    out = bytearray(8 * (L["pwords"] if packing else L["words"]))
    out[:8] = (PACKED_KEY_MAGIC if packing else kref.KEY_MAGIC).to_bytes(8, "little")
    out[8:88] = blob[8:88]
    one = pack_point_bytes if packing else unpack_point_bytes
    sw, dw = (8, 4) if packing else (4, 8)      # words of a source / destination G1 point
    pieces = [(g, (off if packing else poff), (poff if packing else off)) for g, off, poff in FIXED]
    s1, d1, s2, d2 = (L["off_g1"], L["poff_g1"], L["off_g2"], L["poff_g2"]) if packing else (L["poff_g1"], L["off_g1"], L["poff_g2"], L["off_g2"])
    pieces += [(1, s1 + sw * i, d1 + dw * i) for i in range(L["n_g1"])] + [(2, s2 + 2 * sw * i, d2 + 2 * dw * i) for i in range(L["n_g2"])]
    for g, src, dst in pieces:
        o, f = one(g, blob[8 * src:8 * (src + sw * g)])
        if f:
            return None, f, (src, f)
        out[8 * dst:8 * dst + len(o)] = o
    return bytes(out), 0, (0, 0)


def pack_key(blob):
    """(packed bytes or None, bits, first_bad) of vimz_decider_key_pack, or ValueError with its message"""
    return _key(blob, True)


def unpack_key(blob):
    return _key(blob, False)


def key_point_words(shape):
    """name -> (group, word offset in the key, word offset in the packed key) of one point in each part of a key of that shape: the fixed points, the G1 run's
    first, a point inside it and its last, the G2 run's first and last"""
    L = runs(*shape)
    return {"kzg": FIXED[0], "delta1": FIXED[3], "delta2": FIXED[6], "g1_first": (1, L["off_g1"], L["poff_g1"]),
            "g1_inside": (1, L["off_g1"] + 8 * 5, L["poff_g1"] + 4 * 5), "g1_last": (1, L["off_g2"] - 8, L["poff_g2"] - 4),
            "g2_first": (2, L["off_g2"], L["poff_g2"]), "g2_last": (2, L["words"] - 16, L["pwords"] - 8)}


# ---- points and bad encodings -------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 129)
G1_NO_Y = (0, 4, 10, 12)                       # x with x³ + 3 no square
G2_NO_Y = ((0, 0), (0, 2), (1, 1))             # x with x³ + b' no square


@functools.lru_cache(maxsize=None)
def scalars(n, label=""):
    """n scalars: 1, 2, r - 1, then random ones; 0 (the identity) never"""
    rng = random.Random(f"point_pack/{label}/{n}")
    return tuple(([1, 2, R - 1] + [rng.randrange(1, R) for _ in range(max(0, n - 3))])[:n])


@functools.lru_cache(maxsize=None)
def point_bytes(group, s):
    """[s]G as canonical bytes, the identity for s = 0"""
    if s % R == 0:
        return b"\0" * (64 * group)
    return kref.g1_bytes(bp.g1_mul(bp.G1, s % R)) if group == 1 else kref.g2_bytes(bp.g2_mul(bp.G2, s % R))


POOL = 12      # distinct scalars the arrays below draw from: curve arithmetic in Python is the slow part


def array(group, n, identity="none"):
    """n points [s]G over a pool of scalars that holds 1, 2, r - 1 and random ones (so both signs occur from n = 3 on: [s]G and [r - s]G differ in SIGN alone);
    identity: none, first, last or all"""
    pool = scalars(POOL, f"g{group}")
    pts = [point_bytes(group, pool[i % POOL]) for i in range(n)]
    zero = b"\0" * (64 * group)
    if identity == "first":
        pts[0] = zero
    elif identity == "last":
        pts[-1] = zero
    elif identity == "all":
        pts = [zero] * n
    return b"".join(pts)


def bad_packed(group):
    """name -> (packed bytes of ONE point, finding) for the encodings that must not unpack"""
    good = pack_point_bytes(group, point_bytes(group, 5))[0]
    top = lambda data, bits: data[:-1] + bytes([data[-1] | bits])      # noqa: E731
    size = 32 * group
    cases = {"x_is_q": (b"\0" * (size - 32) + Q.to_bytes(32, "little"), COORD),
             "inf_with_sign": (top(b"\0" * size, 0xC0), FLAGS),
             "inf_with_x": (top((1).to_bytes(size, "little"), 0x80), FLAGS),
             "inf_with_good_x": (top(good, 0x80), FLAGS)}
    if group == 1:
        cases.update({f"no_y/{x}": (x.to_bytes(32, "little"), OFF_CURVE) for x in G1_NO_Y})
        cases.update({f"no_y_sign/{x}": (top(x.to_bytes(32, "little"), 0x40), OFF_CURVE) for x in G1_NO_Y})
    else:
        cases.update({f"no_y/{x[0]}_{x[1]}": (x[0].to_bytes(32, "little") + x[1].to_bytes(32, "little"), OFF_CURVE) for x in G2_NO_Y})
        cases["c0_is_q"] = (Q.to_bytes(32, "little") + good[32:], COORD)
        cases["stray_bit_62"] = (good[:31] + bytes([good[31] | 0x40]) + good[32:], FLAGS)
        cases["stray_bit_63"] = (good[:31] + bytes([good[31] | 0x80]) + good[32:], FLAGS)
        cases["stray_bit_and_c1_is_q"] = (good[:31] + bytes([good[31] | 0x80]) + Q.to_bytes(32, "little"), FLAGS | COORD)
        cases["stray_bit_in_inf"] = (b"\0" * 31 + b"\x40" + top(b"\0" * 32, 0x80), FLAGS)
    return cases


def bad_points(group):
    """name -> (bytes of ONE unpacked point, finding) for the points that must not pack"""
    good = point_bytes(group, 5)
    c = _ints(good, 64 * group)
    enc = lambda v: b"".join(x.to_bytes(32, "little") for x in v)      # noqa: E731
    cases = {"x_is_q": (enc([Q] + c[1:]), COORD), "y_is_q": (enc(c[:-1] + [Q]), COORD), "y_off_by_one": (enc(c[:-1] + [(c[-1] + 1) % Q]), OFF_CURVE),
             "y_is_zero": (enc(c[:group] + [0] * group), OFF_CURVE), "x_is_zero": (enc([0] * group + c[group:]), OFF_CURVE)}
    return cases


# ---- the values the device's Fq2 root is run on (vimz_test_fq2_sqrt) -------------------------------------------------------------------------------------------
def sqrt_values():
    """Fq2 values: (a0, 0) with a0 a residue, the non-residue 3 and other non-residues, (0, a1), squares with both parts, non-squares, zero, one"""
    rng = random.Random("point_pack/fq2_sqrt")
    vals = [(0, 0), (1, 0), (4, 0), (3, 0), (Q - 1, 0), (Q - 4, 0), (0, 1), (0, Q - 1), (0, 2), (0, 7)]
    for _ in range(6):
        a = rng.randrange(1, Q)
        vals += [(a * a % Q, 0), ((Q - a * a) % Q, 0), (0, a)]
    for _ in range(8):
        z = (rng.randrange(Q), rng.randrange(1, Q))
        vals += [f2_sqr(z), z]
    while sum(1 for v in vals if not fq2_is_square(v)) < 6:
        vals.append((rng.randrange(Q), rng.randrange(1, Q)))
    vals += [rhs2(x) for x in G2_NO_Y]
    return vals
