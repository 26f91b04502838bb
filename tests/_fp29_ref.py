"""Vectors and an integer reference for the probe of the lazily reduced field (vimz_amd/csrc/fp29_probe.hpp over fp29.hpp).  Test infrastructure.

Plain Python integers only: nothing here comes from oracle/ or from the library.  A value of the 9 x 29-bit representation is the integer
sum(limb_i << 29 i); the Montgomery radix is R = 2^261; the 8 x 32 side (fp.hpp) is a 256-bit integer in its first eight words.

Every operation is given in-contract operands only (the preconditions written in fp29.hpp) and three things are checked of a result:
the value (the exact integer where the operation is exact: add, sub<K>, neg, dbl, canon, the conversions; the residue otherwise), limb
normalisation (each limb < 2^29) and the documented output bound as an exact integer inequality."""
import os
import random
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("BnFr", "BnFq", "PallasFp", "VestaFq")
MODULUS = (
    21888242871839275222246405745257275088548364400416034343698204186575808495617,
    21888242871839275222246405745257275088696311157297823662689037894645226208583,
    28948022309329048855892746252171976963363056481941560715954676764349967630337,
    28948022309329048855892746252171976963363056481941647379679742748393362948097,
)
R = 1 << 261
TOP = 1 << 261                      # every value of the representation is below this
WORDS = 9                           # words per operand / result slot
SUB_K = (1, 2, 3, 4, 6)             # the instantiations of sub<K> the probe knows: test_probe_covers_every_sub_in_the_tree keeps it complete
OPS = {"mul": 0, "sqr": 1, "mul_add2": 2, "add": 3, "neg": 4, "dbl": 5, "weak_reduce": 6, "canon": 7, "is_zero_mod": 8, "unpack": 9, "pack": 10,
       "from_std": 11, "to_std": 12, "r29_of": 13, "fe_of29": 14, "pack_unpack": 15}
OPS.update({f"sub{k}": 100 + k for k in SUB_K})
WORD_RESULT = {"unpack", "to_std", "fe_of29"}       # results in the 8 x 32 form
RANDOM_PER_OP = 20000
LIMIT_PAIRS = ((64, 1), (32, 2), (16, 4), (8, 8), (4, 16), (2, 32), (1, 64))


def sub_instantiations_in_tree():
    """Every K of a `sub<K>` in the library's sources."""
    found = set()
    src = os.path.join(ROOT, "vimz_amd", "csrc")
    for dirpath, _, names in os.walk(src):
        if os.path.basename(dirpath) == "build" or "/build/" in dirpath + "/":
            continue
        for n in names:
            if n.endswith((".hpp", ".hip", ".cpp", ".h")) and n != "fp29_probe.hpp":
                found |= {int(k) for k in re.findall(r"\bsub<\s*(\d+)\s*>", open(os.path.join(dirpath, n), errors="replace").read())}
    return found


# ---- integers <-> word arrays ---------------------------------------------------------------------------------------------------------
def ints_to_limbs29(xs):
    """ints below 2^261 -> (n, 9) uint32 of 29-bit limbs"""
    n = len(xs)
    if n == 0:
        return np.zeros((0, WORDS), dtype=np.uint32)
    w = np.frombuffer(b"".join(int(x).to_bytes(40, "little") for x in xs), dtype="<u8").reshape(n, 5)
    out = np.zeros((n, WORDS), dtype=np.uint32)
    for i in range(9):
        q, off = divmod(29 * i, 64)
        v = w[:, q] >> np.uint64(off)
        if off > 35:
            v = v | (w[:, q + 1] << np.uint64(64 - off))
        out[:, i] = (v & np.uint64(0x1fffffff)).astype(np.uint32)
    return out


def ints_to_words32(xs):
    """ints below 2^256 -> (n, 9) uint32: eight 32-bit words and a zero"""
    n = len(xs)
    out = np.zeros((n, WORDS), dtype=np.uint32)
    if n:
        out[:, :8] = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u4").reshape(n, 8)
    return out


def limbs29_to_ints(a):
    """(n, 9) uint32 -> ints, sum(limb << 29 i) whatever the limbs hold"""
    a = np.asarray(a, dtype=np.uint64)
    lo = a[:, 0] | (a[:, 1] << np.uint64(29)) | ((a[:, 2] & np.uint64(0x3f)) << np.uint64(58))          # bits 0..63 when limbs are normalised
    if (a >> np.uint64(29)).any():                      # not normalised: the slow exact way
        return [sum(int(r[i]) << (29 * i) for i in range(9)) for r in a]
    w = np.zeros((len(a), 5), dtype="<u8")
    for i in range(9):
        q, off = divmod(29 * i, 64)
        w[:, q] |= a[:, i] << np.uint64(off)
        if off > 35:
            w[:, q + 1] |= a[:, i] >> np.uint64(64 - off)
    assert np.array_equal(w[:, 0], lo)
    raw = w.tobytes()
    return [int.from_bytes(raw[40 * i:40 * i + 40], "little") for i in range(len(a))]


def words32_to_ints(a):
    raw = np.ascontiguousarray(np.asarray(a, dtype="<u4")[:, :8]).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(a))]


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def residues(p):
    out = [0, 1, 2, p - 1, p - 2, (p - 1) // 2]
    for k in sorted(set(range(0, 256, 29)) | set(range(0, 256, 32))):
        out += [((1 << k) - 1) % p, (1 << k) % p, ((1 << k) + 1) % p]
    seen, uniq = set(), []
    for x in out:
        if x not in seen:
            seen.add(x); uniq.append(x)
    return uniq


LIMB_SET = (0, 1, 1 << 28, (1 << 29) - 1)
WORD_SET = (0, 1, 0x7fffffff, 0x80000000, 0xffffffff)


def _patterns(rng, choices, n_low, n_random):
    """lists of n_low digits from `choices`: uniform, alternating, one digit different, then random ones"""
    pats = [[c] * n_low for c in choices]
    pats += [[(a, b)[i & 1] for i in range(n_low)] for a in choices for b in choices if a != b]
    pats += [[(b if i == pos else a) for i in range(n_low)] for a in choices for b in choices if a != b for pos in range(n_low)]
    pats += [[rng.choice(choices) for _ in range(n_low)] for _ in range(n_random)]
    return pats


def limb_patterns(rng, limit, n_random=300):
    """integers below `limit` (<= 2^261) whose 29-bit limbs all come from LIMB_SET, but for a top limb lowered where the bound asks for it"""
    out = []
    for low in _patterns(rng, LIMB_SET, 8, n_random):
        base = sum(d << (29 * i) for i, d in enumerate(low))
        tops = set(LIMB_SET)
        if limit > base:
            tops.add(min((limit - 1 - base) >> 232, (1 << 29) - 1))          # the largest top limb the bound allows
        for t in sorted(tops):
            v = base + (t << 232)
            if v < limit:
                out.append(v)
    return out


def word_patterns(rng, p, n_random=300):
    """integers below p whose 32-bit words come from WORD_SET, reduced below p by clearing top bits"""
    out = []
    for ws in _patterns(rng, WORD_SET, 8, n_random):
        v = sum(d << (32 * i) for i, d in enumerate(ws))
        while v >= p:
            v &= (1 << (v.bit_length() - 1)) - 1
        out.append(v)
    return out


def bound_of(x, p):
    """the smallest integer B with x < B p"""
    return x // p + 1


class Block:
    def __init__(self, field, op, operands):
        self.field, self.op, self.operands = field, op, operands          # operands: list of (a, b, c, d) integers

    def __len__(self):
        return len(self.operands)

    def arrays(self):
        conv = ints_to_words32 if self.op in ("pack", "from_std", "r29_of") else ints_to_limbs29
        cols = list(zip(*self.operands)) if self.operands else [[], [], [], []]
        return [conv(cols[0])] + [ints_to_limbs29(c) for c in cols[1:]]


def _lifted_pairs(p, rs):
    """(a, b) with a < Ba p, b < Bb p, Ba Bb <= 64: every lift of a with the largest lift of b it allows and the mirror, residues cycled; then every pair of
    residues at the limit pairs and at (1, 1)"""
    out = []
    n = len(rs)
    for ka in range(64):
        kb = 64 // (ka + 1) - 1
        for i, ra in enumerate(rs):
            rb = rs[(7 * i + ka) % n]
            out.append((ra + ka * p, rb + kb * p)); out.append((rb + kb * p, ra + ka * p))
    for ba, bb in LIMIT_PAIRS + ((1, 1),):
        out += [(ra + (ba - 1) * p, rb + (bb - 1) * p) for ra in rs for rb in rs]
    return out


def operands_for(field, op, rng, n_random=RANDOM_PER_OP):
    p = MODULUS[field]
    rs = residues(p)
    Z = (0, 0)
    ops = []
    if op == "mul":
        ops = [(a, b) + Z for a, b in _lifted_pairs(p, rs)]
        for ba, bb in LIMIT_PAIRS + ((1, 1), (8, 7)):
            pa, pb = limb_patterns(rng, ba * p, 60), limb_patterns(rng, bb * p, 60)
            ops += [(a, pb[(5 * i) % len(pb)]) + Z for i, a in enumerate(pa)] + [(pa[(3 * i) % len(pa)], b) + Z for i, b in enumerate(pb)]
            ops += [(ba * p - 1, bb * p - 1) + Z]                                              # the largest operands of the pair
        for _ in range(n_random):
            ba = rng.randint(1, 64); bb = rng.randint(1, 64 // ba)
            ops.append((rng.randrange(ba * p), rng.randrange(bb * p)) + Z)
    elif op == "sqr":
        ops = [(r + k * p, 0, 0, 0) for r in rs for k in range(8)] + [(a, 0, 0, 0) for a in limb_patterns(rng, 8 * p)] + [(8 * p - 1, 0, 0, 0)]
        ops += [(rng.randrange(8 * p), 0, 0, 0) for _ in range(n_random)]
    elif op == "mul_add2":
        quads = ((32, 1, 32, 1), (1, 32, 1, 32), (8, 4, 4, 8), (63, 1, 1, 1), (1, 1, 1, 63), (7, 8, 8, 1), (4, 8, 2, 16), (1, 1, 1, 1), (2, 16, 16, 2), (1, 63, 1, 1), (5, 5, 6, 6))
        n = len(rs)
        for q in quads:
            for i in range(n):
                for j in (0, 1, 3, 5, 11):
                    ops.append(tuple(rs[(i + s * j + s) % n] + (b - 1) * p for s, b in enumerate(q)))
            pats = [limb_patterns(rng, b * p, 40) for b in q]
            for i in range(max(len(t) for t in pats)):
                ops.append(tuple(t[(i * (s + 1)) % len(t)] for s, t in enumerate(pats)))
            ops.append(tuple(b * p - 1 for b in q))
        for _ in range(n_random):
            s1 = rng.randint(1, 63); s2 = 64 - s1
            ba = rng.randint(1, s1); bb = s1 // ba; bc = rng.randint(1, s2); bd = s2 // bc
            ops.append((rng.randrange(ba * p), rng.randrange(bb * p), rng.randrange(bc * p), rng.randrange(bd * p)))
    elif op == "add":
        ops = [((1 << 232) - 1, 1), (TOP - 2, 1), (1 << 260, (1 << 260) - 1), ((1 << 260) - 1, (1 << 260) - 1), (0, 0), (TOP - 1, 0), (0, TOP - 1),
               (sum(((1 << 29) - 1) << (29 * i) for i in range(0, 9, 2)), sum(((1 << 29) - 1) << (29 * i) for i in range(1, 9, 2))), ((1 << 260) - 1, 1), ((1 << 29) - 1, 1)]
        kmax = TOP // p - 1                                     # r + k p < 2^261 for every residue r
        ops += [(ra + ka * p, rs[(3 * i + ka) % len(rs)] + (kmax - 1 - ka) * p) for ka in range(kmax) for i, ra in enumerate(rs)]
        pats = limb_patterns(rng, TOP)
        ops += [(a, b) for i, a in enumerate(pats) for b in (pats[(11 * i + 1) % len(pats)], 1, TOP - 1 - a) if a + b < TOP]
        for _ in range(n_random):
            a = rng.randrange(TOP); ops.append((a, rng.randrange(TOP - a)))
        ops = [o + Z for o in ops]
    elif op.startswith("sub"):
        k = int(op[3:])
        amax = TOP - k * p                                       # a + K p < 2^261
        ops = [(0, 0), (0, k * p - 1), (amax - 1, 0), (amax - 1, k * p - 1), (0, 1), (1 << 232, 1), (1 << 232, k * p - 1)]
        ka_max = amax // p - 1
        for ka in sorted(set(range(0, min(ka_max, 12))) | {ka_max - 1, ka_max}):
            for i, ra in enumerate(rs):
                for kb in range(k):
                    ops.append((ra + ka * p, rs[(5 * i + kb + ka) % len(rs)] + kb * p))
        pa, pb = limb_patterns(rng, amax), limb_patterns(rng, k * p)
        ops += [(a, pb[(7 * i) % len(pb)]) for i, a in enumerate(pa)] + [(pa[(13 * i) % len(pa)], b) for i, b in enumerate(pb)]
        ops += [(rng.randrange(amax if i & 1 else 8 * p), rng.randrange(k * p)) for i in range(n_random)]
        ops = [o + Z for o in ops]
    elif op == "neg":
        ops = [(r, 0, 0, 0) for r in rs + [p]] + [(a, 0, 0, 0) for a in limb_patterns(rng, p + 1)] + [(rng.randrange(p + 1), 0, 0, 0) for _ in range(n_random)]
    elif op == "dbl":
        half = TOP // 2
        ops = [(r + k * p, 0, 0, 0) for r in rs for k in range(half // p - 1)] + [(a, 0, 0, 0) for a in limb_patterns(rng, half)] + [(half - 1, 0, 0, 0)]
        ops += [(rng.randrange(half), 0, 0, 0) for _ in range(n_random)]
    elif op in ("weak_reduce", "fe_of29"):
        vals = [TOP - 1] + [q << 253 for q in range(256)] + [(q << 253) + (1 << 253) - 1 for q in range(256)]
        vals += [r + k * p for r in rs for k in range(TOP // p - 1)] + [k * p for k in range(TOP // p + 1) if k * p < TOP] + limb_patterns(rng, TOP)
        vals += [rng.randrange(TOP) for _ in range(n_random)]
        ops = [(v, 0, 0, 0) for v in vals]
    elif op in ("canon", "to_std"):
        vals = [r + k * p for r in rs for k in range(8)] + [k * p for k in range(8)] + [k * p - 1 for k in range(1, 9)] + [k * p + 1 for k in range(8)] + limb_patterns(rng, 8 * p)
        vals += [rng.randrange(8 * p) for _ in range(n_random)]
        ops = [(v, 0, 0, 0) for v in vals]
    elif op == "is_zero_mod":
        vals = [k * p for k in range(8)] + [k * p - 1 for k in range(1, 9)] + [k * p + 1 for k in range(8)] + [r + k * p for r in rs for k in range(8)] + limb_patterns(rng, 8 * p)
        # values that pass the first test (k = v0 / p mod 2^29 below 8) without being multiples of p: k p with one higher limb changed
        for k in range(8):
            for i in range(1, 9):
                for delta in (1 << (29 * i), -(1 << (29 * i))):
                    v = k * p + delta
                    if 0 <= v < 8 * p:
                        vals.append(v)
        vals += [rng.randrange(8 * p) for _ in range(n_random // 2)] + [rng.randrange(8) * p for _ in range(n_random // 4)]
        vals += [rng.randrange(8) * p + (rng.randrange(1, 1 << 24) << (29 * rng.randrange(1, 8))) for _ in range(n_random - n_random // 2 - n_random // 4)]
        assert all(v < 8 * p for v in vals)
        ops = [(v, 0, 0, 0) for v in vals]
    elif op in ("unpack", "pack_unpack"):
        lim = 1 << 256
        vals = rs + [lim - 1, lim - 2, 1 << 255, p, 2 * p] + limb_patterns(rng, lim) + [rng.randrange(lim) for _ in range(n_random)]
        ops = [(v, 0, 0, 0) for v in vals]
    elif op == "pack":
        lim = 1 << 256
        pats = [sum(d << (32 * i) for i, d in enumerate(ws)) for ws in _patterns(rng, WORD_SET, 8, 300)]
        vals = rs + [lim - 1, lim - 2, 1 << 255, p, 2 * p] + pats + limb_patterns(rng, lim) + [rng.randrange(lim) for _ in range(n_random)]
        ops = [(v, 0, 0, 0) for v in vals]
    elif op in ("from_std", "r29_of"):
        vals = rs + word_patterns(rng, p) + limb_patterns(rng, p) + [rng.randrange(p) for _ in range(n_random)]
        ops = [(v, 0, 0, 0) for v in vals]
    else:
        raise KeyError(op)
    return ops


def all_blocks(n_random=RANDOM_PER_OP, fields=(0, 1, 2, 3), ops=None):
    blocks = []
    for f in fields:
        for op in (ops or sorted(OPS, key=OPS.get)):
            rng = random.Random(f"fp29:{f}:{op}")
            blocks.append(Block(f, op, operands_for(f, op, rng, n_random)))
    return blocks


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def in_contract(field, op, a, b, c, d):
    """the precondition of `op` as fp29.hpp writes it"""
    p = MODULUS[field]
    B = lambda x: bound_of(x, p)
    if max(a, b, c, d) >= TOP or min(a, b, c, d) < 0:
        return False
    if op == "mul":
        return B(a) * B(b) <= 64
    if op == "sqr":
        return B(a) * B(a) <= 64
    if op == "mul_add2":
        return B(a) * B(b) + B(c) * B(d) <= 64
    if op == "add":
        return a + b < TOP
    if op.startswith("sub"):
        k = int(op[3:])
        return b < k * p and a + k * p < TOP
    if op == "neg":
        return a <= p
    if op == "dbl":
        return 2 * a < TOP
    if op in ("canon", "to_std", "is_zero_mod"):
        return a < 8 * p
    if op in ("unpack", "pack", "pack_unpack"):
        return a < (1 << 256)
    if op in ("from_std", "r29_of"):
        return a < p
    return True             # weak_reduce, fe_of29: anything below 2^261


def check_one(field, op, a, b, c, d, got, limbs_ok):
    """None, or what is wrong with the result `got` (an integer) of `op`"""
    p = MODULUS[field]
    if op not in WORD_RESULT and not limbs_ok:
        return "a limb is not below 2^29"
    if op == "mul" or op == "sqr":
        if op == "sqr":
            b = a
        if (got * R - a * b) % p:
            return "residue"
        if not 128 * got < (bound_of(a, p) * bound_of(b, p) + 128) * p:
            return "bound (Ba Bb / 128 + 1) p"
        if not got * R < a * b + p * R:
            return "bound (a b) / 2^261 + p"
    elif op == "mul_add2":
        if (got * R - a * b - c * d) % p:
            return "residue"
        s = bound_of(a, p) * bound_of(b, p) + bound_of(c, p) * bound_of(d, p)
        if not 128 * got < (s + 128) * p:
            return "bound ((Ba Bb + Bc Bd) / 128 + 1) p"
        if not 2 * got < 3 * p:
            return "bound 1.5 p"
    elif op == "add":
        if got != a + b:
            return "not the integer a + b"
    elif op.startswith("sub"):
        k = int(op[3:])
        if got != a - b + k * p:
            return f"not the integer a - b + {k} p"
        if not got < (bound_of(a, p) + k) * p:
            return "bound (Ba + K) p"
    elif op == "neg":
        if got != p - a:
            return "not p - a"
    elif op == "dbl":
        if got != 2 * a:
            return "not 2 a"
    elif op == "weak_reduce":
        if (got - a) % p:
            return "residue"
        if got > a:
            return "grew"
        if not got < 3 * p:
            return "bound 3 p"
        if field < 2 and not 10 * got < 19 * p:
            return "bound 1.9 p (BN254)"
    elif op in ("canon", "fe_of29"):
        if got != a % p:
            return "not a mod p"
    elif op == "is_zero_mod":
        if got != (1 if a % p == 0 else 0):
            return "predicate"
    elif op in ("unpack", "pack", "pack_unpack"):
        if got != a:
            return "not the same integer"
    elif op in ("from_std", "r29_of"):
        if got != (a << 5) % p:
            return "not 32 a mod p"
    elif op == "to_std":
        if got != a * pow(32, -1, p) % p:
            return "not a / 32 mod p"
    else:
        return "unknown operation"
    return None


def check_block(block, out, where="host"):
    """asserts every result of one block; returns the number of cases checked"""
    out = np.asarray(out, dtype=np.uint32).reshape(-1, WORDS)
    assert len(out) == len(block), (FIELDS[block.field], block.op, len(out), len(block))
    op = block.op
    if op in WORD_RESULT:
        got = words32_to_ints(out)
        ok = out[:, 8] == 0
    else:
        got = limbs29_to_ints(out)
        ok = (out >> np.uint32(29) == 0).all(axis=1)
    for i, (opnd, g) in enumerate(zip(block.operands, got)):
        assert in_contract(block.field, op, *opnd), f"generator: out-of-contract operand for {FIELDS[block.field]} {op} #{i}: {[hex(x) for x in opnd]}"
        err = check_one(block.field, op, *opnd, g, bool(ok[i]))
        assert err is None, f"{where}: {FIELDS[block.field]} {op} case {i}: {err}; operands {[hex(x) for x in opnd]} result {hex(g)} words {[hex(int(x)) for x in out[i]]}"
    return len(block)


def write_blocks(blocks, path):
    with open(path, "wb") as f:
        for b in blocks:
            np.array([b.field, OPS[b.op], len(b)], dtype="<u4").tofile(f)
            for arr in b.arrays():
                arr.astype("<u4").tofile(f)


def read_results(blocks, path):
    raw = np.fromfile(path, dtype="<u4")
    assert raw.size == WORDS * sum(len(b) for b in blocks), "result file has the wrong size"
    outs, at = [], 0
    for b in blocks:
        outs.append(raw[at:at + WORDS * len(b)].reshape(-1, WORDS)); at += WORDS * len(b)
    return outs


def build_host_probe(workdir, extra_flags=(), csrc=None):
    import subprocess
    exe = os.path.join(str(workdir), "fp29_probe_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", *extra_flags, "-I", csrc or os.path.join(ROOT, "vimz_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "fp29_probe_host.cpp")])
    return exe


def run_host_probe(exe, blocks, workdir):
    import subprocess
    src, dst = os.path.join(str(workdir), "fp29_in.bin"), os.path.join(str(workdir), "fp29_out.bin")
    write_blocks(blocks, src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return read_results(blocks, dst)
