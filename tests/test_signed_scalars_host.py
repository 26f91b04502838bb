"""The signed scalar loader of the MSM (vimz_amd/csrc/msm.hpp: load_scalar with `sgn`, then for_each_digit / signed_digit) as a model in
Python integers: a canonical scalar above (p - 1)/2 enters the recoding as p - s with a flip flag, and the flip negates every digit.
Checked for every window the pipeline uses (7: the fused small path, 11 / 13 / 15 / 16: the large one) over the four scalar fields:
the digits spell +-s modulo p, stay inside the bucket range, and a "negative small" value costs the digits of the small value.
The reference is Python's arithmetic throughout; nothing here calls the library."""
import os
import random
import re

import pytest

FIELDS = {
    "BnFr": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
    "BnFq": 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47,
    "PallasFp": 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
    "VestaFq": 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
}
WINDOWS = [7, 11, 13, 15, 16]


def windows_of(p, c):
    """msm_plan: K = ceil((bits + 1) / c)"""
    return (p.bit_length() + 1 + c - 1) // c


def load_signed(s, p, sgn=True):
    """load_scalar's choice: (value handed to the recoding, flip).  A word that is not below p is left alone."""
    if sgn and s < p and s > (p - 1) // 2:
        return p - s, 1
    return s, 0


def digits_walk(s, c, K):
    """for_each_digit: the carry walk from window 0 up"""
    half, carry, out = 1 << (c - 1), 0, []
    for w in range(K):
        d = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        neg = d > half
        out.append(d - (1 << c) if neg else d)
        carry = 1 if neg else 0
    return out, carry


def digit_direct(s, c, w):
    """signed_digit: window w alone — the carry into it is one exactly when the low c*w bits exceed the threshold Σ_{j<w} half·2^(cj)"""
    half = 1 << (c - 1)
    thr = sum(half << (c * j) for j in range(w))
    carry = 1 if (s & ((1 << (c * w)) - 1)) > thr else 0
    d = ((s >> (w * c)) & ((1 << c) - 1)) + carry
    return d - (1 << c) if d > half else d


def boundary_values(p):
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (p - 1) // 2 - 1, (p + 1) // 2 + 1]
    for k in range(p.bit_length()):
        if (1 << k) < p:
            vals += [1 << k, p - (1 << k)]
    return vals


def check(s, p, c):
    K = windows_of(p, c)
    half = 1 << (c - 1)
    v, flip = load_signed(s, p)
    assert 0 <= v <= (p - 1) // 2
    dig, carry = digits_walk(v, c, K)
    assert carry == 0, "the top window must absorb the last carry"
    assert all(-(half - 1) <= d <= half for d in dig)
    assert sum(d << (c * w) for w, d in enumerate(dig)) == v
    emitted = [-d if flip else d for d in dig]                       # what reaches the buckets: |digit| - 1 indexes a bucket, the sign is a bit
    assert all(1 <= abs(d) <= half for d in emitted if d)
    assert sum(d << (c * w) for w, d in enumerate(emitted)) % p == s % p
    return dig


def test_moduli_are_the_library_s():
    """the four moduli of this model against the field definitions the kernels are compiled from"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vimz_amd", "csrc", "fp.hpp")).read()
    for name, p in FIELDS.items():
        m = re.search(r"VZ_FIELD\(" + name + r",([^)]*)\)", src)
        assert m, name
        words = [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")]
        assert len(words) == 8 and sum(w << (32 * (7 - i)) for i, w in enumerate(words)) == p
        assert p % 2 == 1 and p.bit_length() in (254, 255)


@pytest.mark.parametrize("name", sorted(FIELDS))
@pytest.mark.parametrize("c", WINDOWS)
def test_boundary_values(name, c):
    p = FIELDS[name]
    for s in boundary_values(p):
        check(s, p, c)
    K = windows_of(p, c)
    # p - 1 is ONE negative digit of magnitude one; (p - 1)/2 is the largest value taken as it is, (p + 1)/2 the first one negated
    v, flip = load_signed(p - 1, p)
    assert (v, flip) == (1, 1) and digits_walk(v, c, K)[0] == [1] + [0] * (K - 1)
    assert load_signed((p - 1) // 2, p) == ((p - 1) // 2, 0)
    assert load_signed((p + 1) // 2, p) == ((p - 1) // 2, 1)
    assert load_signed(0, p) == (0, 0) and load_signed(1, p) == (1, 0)
    # words that are not canonical are not touched (as without the switch)
    assert load_signed(p, p) == (p, 0) and load_signed((1 << 256) - 1, p) == ((1 << 256) - 1, 0)
    # the switch off: the plain recoding
    assert load_signed(p - 1, p, sgn=False) == (p - 1, 0)


@pytest.mark.parametrize("name", sorted(FIELDS))
@pytest.mark.parametrize("c", WINDOWS)
def test_random_values_and_small_negatives(name, c):
    p = FIELDS[name]
    rng = random.Random(1000 * c + len(name))
    K = windows_of(p, c)
    for _ in range(10000):
        check(rng.randrange(p), p, c)
    top = -(-(139 + 1) // c)                                         # windows a value below 2^139 can reach (one more bit for the carry)
    for _ in range(2000):
        x = rng.getrandbits(139) | 1
        small = check(x, p, c)
        neg = check(p - x, p, c)
        assert neg == small                                          # the same digits, the flip aside
        assert all(d == 0 for d in small[top:]) and sum(1 for d in small if d) <= top
        if name.startswith("Bn"):                                    # without the loader: a dense number (the Pasta moduli are 2^254 + a 126-bit tail,
            plain, _ = digits_walk(p - x, c, K)                      # and the run of ones below 2^254 recodes to zeros by itself)
            assert sum(1 for d in plain if d) > top


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_direct_digit_of_the_fused_kernels(name):
    """signed_digit (one window without the walk below it), c = 7: the same digits as the walk, on flipped and unflipped values"""
    p = FIELDS[name]
    rng = random.Random(7 + len(name))
    K = windows_of(p, 7)
    vals = boundary_values(p) + [rng.randrange(p) for _ in range(3000)] + [p - rng.getrandbits(139) for _ in range(500)]
    for s in vals:
        v, _ = load_signed(s, p)
        dig, _ = digits_walk(v, 7, K)
        assert [digit_direct(v, 7, w) for w in range(K)] == dig


def test_cross_term_values_at_the_bench_window():
    """What the step rows' commitment sees on a boolean row whose fresh bit is one: 2(a - u) with u = 1 + Σ r_k, a = Σ_{b_k = 1} r_k and
    r_k = 2^128 | rho_k.  At c = 15 the field element has 17 non-zero digits, seven of them (windows 10..16) the same for every such
    scalar; taken as a negative it has at most ten and nothing above window 9."""
    p, c = FIELDS["BnFr"], 15
    K = windows_of(p, c)
    assert K == 17
    rng = random.Random(2026)
    tops = set()
    for steps in (20, 256, 720):
        r = [(1 << 128) | rng.getrandbits(128) for _ in range(steps)]
        for _ in range(300):
            u = 1 + sum(r)
            a = sum(x for x in r if rng.random() < 0.5)
            s = (2 * (a - u)) % p
            assert s > (p - 1) // 2
            plain, _ = digits_walk(s, c, K)
            assert sum(1 for d in plain if d) == 17
            tops.add(tuple(plain[10:]))
            dig = check(s, p, c)
            assert sum(1 for d in dig if d) <= 10 and all(d == 0 for d in dig[10:])
    assert len(tops) == 1
