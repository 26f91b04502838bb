"""Adversarial shapes and values for the SpMV / cross-term seam (vimz_r1cs_upload, vimz_spmv3, vimz_commit_T, vimz_r1cs_check_relaxed, vimz_vec_axpy) and
for the two step-critical kernels behind the test hooks, with a reference that is plain Python integers.  Test infrastructure.

The kernels choose their path per (matrix, row) by its number of terms — one thread (<= SPMV_LONG = 6), sixteen lanes (<= SPMV_MED = 32), a wave — and
skip multiplications by wave ballots over the classes of a term's value {0, 1, anything} and coefficient {1, p - 1, anything}.  So a shape here is a list of
term counts per matrix, and every term is given a (value class, coefficient class) pair laid out so that some waves are uniform in one pair and some hold
every pair: the value class of column c is c mod 5 (what the `cross` assignment realises), a term asks for its class through the column it names.
The layout goes by wave step (wave_step) and relies on the order of a row's own terms, which the upload keeps; wave_census counts what came of it."""
import random

import numpy as np

SPMV_LONG, SPMV_MED = 6, 32                     # vimz_amd/csrc/r1cs_ops.hpp
STAGGER = (0, 1, 5, 6, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 2047, 2048, 2049, 4097, 70000)
CROSS16 = (0, 1, 5, 6, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 254, 255, 256, 257, 2049)
Z_KINDS = ("zero", "one", "pm1", "maxword", "random", "witness", "cross")
FILL = 0x0123456789abcdef0fedcba987654321a5a5a5a55a5a5a5a00000000deadbeef      # what output vectors hold before a call (below every modulus)


def to_limbs(vals):
    """ints -> (n, 4) uint64 (bytes at once: the vectors here run to half a million elements)"""
    vals = list(vals)
    if not vals:
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def from_limbs(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


class Shape:
    """A caller's R1CS shape as three triplet lists (row, col, canonical integer value), shuffled."""

    def __init__(self, name, p, nrows, ncols, mats, lens, layout="seam"):
        self.name, self.p, self.nrows, self.ncols, self.mats, self.lens, self.layout = name, p, nrows, ncols, mats, lens, layout

    @property
    def nnz(self):
        return sum(len(m) for m in self.mats)

    def coo(self, m, mont=False):
        t = self.mats[m]
        k = (1 << 256) % self.p if mont else 1
        return (np.asarray([x[0] for x in t], dtype=np.uint32), np.asarray([x[1] for x in t], dtype=np.uint32), to_limbs([x[2] * k % self.p for x in t]))

    def csr(self, m):
        """(row_ptr, col, val limbs) in the row order a stable sort gives: the oracle's input"""
        t = sorted(self.mats[m], key=lambda x: x[0])
        rp = np.zeros(self.nrows + 1, dtype=np.uint32)
        for r, _, _ in t:
            rp[r + 1] += 1
        return np.cumsum(rp).astype(np.uint32), np.asarray([x[1] for x in t], dtype=np.uint32), to_limbs([x[2] for x in t])

    def expect_info(self):
        counts = [[0] * self.nrows for _ in range(3)]
        for m in range(3):
            for r, _, _ in self.mats[m]:
                counts[m][r] += 1
        items = [c for m in range(3) for c in counts[m] if c > SPMV_LONG]
        return {"nrows": self.nrows, "ncols": self.ncols, "nnz_a": len(self.mats[0]), "nnz_b": len(self.mats[1]), "nnz_c": len(self.mats[2]),
                "dict": len({v for m in self.mats for _, _, v in m}), "n_long": len(items), "n_med": sum(1 for c in items if c <= SPMV_MED)}

    def spmv(self, m, z):
        """row sums of matrix m over the integers z, reduced: duplicates add, a zero coefficient adds nothing"""
        out = [0] * self.nrows
        for r, c, v in self.mats[m]:
            out[r] += v * z[c]
        p = self.p
        return [x % p for x in out]

    def products(self, z):
        return [self.spmv(m, z) for m in range(3)]


def cross_term(p, a1, b1, c1, u1, a2, b2, c2, u2):
    return [(x1 * y2 + x2 * y1 - u1 * w2 - u2 * w1) % p for x1, y1, w1, x2, y2, w2 in zip(a1, b1, c1, a2, b2, c2)]


def _coef(p, cls, rng):
    return (1, p - 1, 0, 2, None)[cls] if cls != 4 else rng.randrange(3, p - 1)


def _keff(lens, dup_rows):
    """term counts after the duplicates: a duplicated row has one term more"""
    return [[k + (1 if r in dup_rows and k else 0) for r, k in enumerate(l)] for l in lens]


def _med_index(counts):
    """(matrix, row) -> position among the sixteen-lane items, in the order the upload lists them (matrix-major, rows ascending)"""
    out, q = {}, 0
    for m in range(3):
        for r, k in enumerate(counts[m]):
            if SPMV_LONG < k <= SPMV_MED:
                out[m, r] = q; q += 1
    return out


def wave_step(layout, counts, med, m, r, j):
    """The wave step that term j (in upload order) of row r of matrix m is processed in, and its lane there: (path, wave, step), lane.  One ballot of a
    kernel is taken over the live lanes of one such step.
      seam layout   one thread per row (<= SPMV_LONG terms): 64 consecutive (matrix, row) threads at the same term index;
                    sixteen lanes per item (<= SPMV_MED): four consecutive items of the host's list, terms 16 t .. 16 t + 15 of each;
                    a wave per item: terms 64 t .. 64 t + 63.
      cross16       sixteen lanes per row, four consecutive rows a wave, matrix after matrix, terms 16 s .. 16 s + 15 of each row a step."""
    k, nrows = counts[m][r], len(counts[0])
    if layout == "cross16":
        return ("cross16", r // 4, (m, j // 16)), 16 * (r % 4) + j % 16
    if k <= SPMV_LONG:
        i = m * nrows + r
        return ("thread", i // 64, j), i % 64
    if k <= SPMV_MED:
        q = med[m, r]
        return ("quad", q // 4, j // 16), 16 * (q % 4) + j % 16
    return ("wave", (m, r), j // 64), j % 64


def _term_pair(rng, layout, counts, med, m, r, j):
    """the (value class, coefficient class) pair, 0..24, of term j of row r of matrix m: by wave step, a third of the steps uniform in one pair, a third
    with every pair lane by lane, a third random"""
    (path, wave, step), lane = wave_step(layout, counts, med, m, r, j)
    h = (sum(wave) if isinstance(wave, tuple) else wave) + (sum(step) if isinstance(step, tuple) else step)
    mode = h % 3
    st = sum(step) if isinstance(step, tuple) else step
    return (7 * (h // 3) + 11 * m + 13 * st) % 25 if mode == 0 else lane % 25 if mode == 1 else rng.randrange(25)


def make_shape(name, p, lens, ncols, seed, ones=False, dup_rows=(), shuffle="rows", layout="seam"):
    """lens = three lists of term counts per row.  ones: every coefficient 1 (the largest lazy sums).  dup_rows: rows whose last term repeats the (row, col)
    of their first.  shuffle: "rows" interleaves the rows' triplets at random but keeps the order of a row's own terms — the upload's counting sort keeps
    it too, so the classes stay where the layout put them; "all" shuffles everything (the order inside a row is then arbitrary)."""
    rng = random.Random(f"seam:{name}:{seed}")
    nrows = len(lens[0])
    assert all(len(l) == nrows for l in lens) and nrows >= 1 and ncols >= 1
    counts = _keff(lens, dup_rows)
    med = _med_index(counts)
    mats = []
    for m in range(3):
        rows = []
        for r, k in enumerate(counts[m]):
            t = []
            for j in range(k):
                vcls, ccls = divmod(_term_pair(rng, layout, counts, med, m, r, j), 5)
                if ncols >= 10:
                    col = 5 * rng.randrange(ncols // 5) + vcls
                    if j == 0 and r % 3 == 0 and (ncols - 1) % 5 == vcls:
                        col = ncols - 1                     # the last column is named too
                else:
                    col = rng.randrange(ncols)
                if j == k - 1 and r in dup_rows and k > 1:
                    col = t[0][1]                           # a duplicate (row, col): the two add
                t.append((r, col, 1 if ones else _coef(p, ccls, rng)))
            rows.append(t)
        if shuffle == "all":
            t = [x for row in rows for x in row]
            rng.shuffle(t)
        else:
            order = [r for r, row in enumerate(rows) for _ in row]
            rng.shuffle(order)
            at = [0] * nrows
            t = []
            for r in order:
                t.append(rows[r][at[r]]); at[r] += 1
        assert all(0 <= r < nrows and 0 <= c < ncols and 0 <= v < p for r, c, v in t)
        mats.append(t)
    return Shape(name, p, nrows, ncols, mats, counts, layout)


def coef_class(p, v):
    return {1: 0, p - 1: 1, 0: 2, 2: 3}.get(v, 4)


def wave_census(shape):
    """What the ballots of the kernels see on this shape under the `cross` assignment (value class of column c = c mod 5), on the term order the upload
    produces (a stable sort by row): per kernel path, the number of wave steps with at least 8 live lanes, of them those uniform in ONE (value,
    coefficient) pair — with the pairs that occur — and those that hold every value class and every coefficient class."""
    med = _med_index(shape.lens)
    steps = {}
    for m in range(3):
        at = [0] * shape.nrows
        for r, c, v in shape.mats[m]:
            key, _ = wave_step(shape.layout, shape.lens, med, m, r, at[r])
            at[r] += 1
            steps.setdefault(key, []).append((c % 5, coef_class(shape.p, v)))
    out = {}
    for (path, _, _), pairs in steps.items():
        if len(pairs) < 8:
            continue
        d = out.setdefault(path, {"steps": 0, "uniform": 0, "uniform_pairs": set(), "every_class": 0})
        d["steps"] += 1
        if len(set(pairs)) == 1:
            d["uniform"] += 1; d["uniform_pairs"].add(pairs[0])
        if len({a for a, _ in pairs}) == 5 and len({b for _, b in pairs}) == 5:
            d["every_class"] += 1
    return out


def _short(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(0, SPMV_LONG + 1) if (r // 64) % 2 else (r % 7) for r in range(n)]


def shapes(p, seed):
    """every shape of the seam test for one field"""
    n = len(STAGGER)
    tail = 384 - n                                      # short rows behind the staggered ones: whole waves of the one-thread kernel
    stag = [[STAGGER[(i + 7 * m) % n] for i in range(n)] + _short(tail, f"{seed}:{m}") for m in range(3)]
    out = [make_shape("staggered", p, stag, 5000, seed, dup_rows=(30, 40, 100))]
    out.append(make_shape("ones", p, [[70000, 3, 2049], [2049, 0, 33], [0, 70000, 7]], 4099, seed, ones=True))
    med = ([7, 32, 16, 9], [8, 31, 7, 20], [12, 7, 32, 32])
    out.append(make_shape("medium_only_nmed0", p, med, 64, seed))
    for k in (1, 2, 3):
        extra = ([10], [11 if k >= 2 else 3], [12 if k >= 3 else 0])
        out.append(make_shape(f"nmed{k}", p, [a + b for a, b in zip(med, extra)], 64, seed))
    cyc = (7, 32, 16, 9, 8, 31, 20, 12, 24, 17, 15, 28)
    out.append(make_shape("quads", p, [[cyc[(r + 5 * m) % len(cyc)] for r in range(64)] for m in range(3)], 500, seed))      # 48 waves of four sixteen-lane items
    out.append(make_shape("wave_only", p, [[33, 64, 100], [65, 33, 200], [128, 40, 33]], 200, seed))
    out.append(make_shape("one_row", p, [[3], [40], [0]], 50, seed))
    r257 = [_short(257, f"{seed}:r257:{m}") for m in range(3)]
    r257[0][255], r257[1][256], r257[2][0] = 20, 70, 9
    out.append(make_shape("rows257", p, r257, 300, seed, dup_rows=(2, 255, 256)))
    out.append(make_shape("shuffled", p, r257, 300, seed, dup_rows=(2, 255, 256), shuffle="all"))          # triplets in any order at all
    out.append(make_shape("one_col", p, [[1, 7, 70], [0, 6, 33], [2, 2, 2]], 1, seed))
    out.append(make_shape("empty_C", p, [[1, 7, 70, 4], [0, 6, 33, 5], [0, 0, 0, 0]], 40, seed))
    return out


def cross16_shape(p, seed):
    """rows for k_spmv_cross16 (sixteen lanes a row, 64 terms a round): the boundary counts, 254..257 terms, and a number of rows that is not a multiple of 16"""
    n = len(CROSS16)
    lens = [[CROSS16[(i + 7 * m) % n] for i in range(n)] + _short(61, f"{seed}:x16:{m}") for m in range(3)]
    return make_shape("cross16", p, lens, 1000, seed, dup_rows=(25, 30), layout="cross16")


def z_vector(kind, p, n, seed):
    rng = random.Random(f"z:{kind}:{seed}")
    if kind == "zero":
        return [0] * n
    if kind == "one":
        return [1] * n
    if kind == "pm1":
        return [p - 1] * n
    if kind == "maxword":                       # the element whose STORED (Montgomery, R = 2^256) word is p - 1: the largest term a lazy sum can be given
        return [(p - 1) * pow(1 << 256, -1, p) % p] * n
    if kind == "random":
        return [rng.randrange(p) for _ in range(n)]
    if kind == "witness":
        return [(0, 1, 0, 1, 0, 1, 0, 1, 255, rng.randrange(p))[rng.randrange(10)] for _ in range(n)]
    if kind == "cross":
        return [(0, 1, p - 1, 2, rng.randrange(3, p - 1))[c % 5] for c in range(n)]
    raise KeyError(kind)


def sat_shape(p, seed, nrows=300):
    """A shape whose row r of C is one reserved column (coefficient 1) that A and B never name: any assignment of the other columns is completed to a
    satisfied one by z[base + r] = az_r bz_r / u.  Returns (shape, base)."""
    base = 200
    lens = [_short(nrows, f"{seed}:sat:{m}") for m in range(2)]
    lens[0][0], lens[1][0], lens[0][nrows - 1], lens[1][255], lens[0][256] = 9, 40, 70, 12, 3
    lens = [[max(1, k) for k in l] for l in lens]
    s = make_shape("sat", p, lens + [[0] * nrows], base, seed)
    s.mats[2] = [(r, base + r, 1) for r in range(nrows)]
    random.Random(f"{seed}:satc").shuffle(s.mats[2])
    s.ncols = base + nrows
    s.lens[2] = [1] * nrows
    return s, base


def satisfy(shape, base, z, u):
    """completes z (the first `base` columns) so that az∘bz = u·cz row by row; u != 0"""
    z = list(z[:base]) + [0] * shape.nrows
    az, bz = shape.spmv(0, z), shape.spmv(1, z)
    inv = pow(u, -1, shape.p)
    for r in range(shape.nrows):
        z[base + r] = az[r] * bz[r] * inv % shape.p
    return z


def unsat_rows(p, az, bz, cz, u, E=None):
    return [i for i in range(len(az)) if (az[i] * bz[i] - u * cz[i] - (E[i] if E is not None else 0)) % p]


def scalars(p, seed):
    """the values a scalar's fast paths branch on, and one that takes the general path"""
    return (0, 1, p - 1, random.Random(f"u:{seed}").randrange(2, p - 1))


def sub3_limit_case(p, seed, nrows=21):
    """Rows on which k_spmv_cross16's last subtraction needs all of its 3 p (r1cs_ops.hpp: T = t1 - t2 + 3 p with t2 = u1·cz2 + cz1 below 2.5 p when the
    fresh u is one): az2 = bz2 = 0 makes t1 the integer 0, and u1, cz2, cz1 are chosen so that the unreduced Montgomery product u1·cz2 comes out above
    p and the stored word of cz1 is p - 1, hence t2 > 2 p.  Every value is an ordinary field element: nothing here is outside the kernel's contract.
    Returns (shape, z, [az1, bz1, cz1], u1): A and B empty, row r of C the single term (r, r, 1)."""
    rng = random.Random(f"sub3:{seed}")
    R29, R32 = 1 << 261, 1 << 256
    pinv = pow(p, -1, R29)
    redc = lambda a, b: (a * b + ((-a * b * pinv) % R29) * p) >> 261          # Fp29::mul without a final subtraction
    while True:
        a = p - 1 - rng.randrange(1 << 200)                                      # r29_of(u1): u1·2^261 mod p, near p
        bs = []
        for _ in range(200000):
            b = p - 1 - rng.randrange(1 << 240)                                  # the stored word of cz2
            if redc(a, b) + (p - 1) > 2 * p:
                bs.append(b)
                if len(bs) == nrows:
                    break
        if len(bs) == nrows:
            break
    inv32, inv29 = pow(R32, -1, p), pow(R29, -1, p)
    u1 = a * inv29 % p
    z = [b * inv32 % p for b in bs]
    shape = Shape("sub3_limit", p, nrows, nrows, [[], [], [(r, r, 1) for r in range(nrows)]], [[0] * nrows, [0] * nrows, [1] * nrows])
    run = [[rng.randrange(p) for _ in range(nrows)], [rng.randrange(p) for _ in range(nrows)], [(p - 1) * inv32 % p] * nrows]
    for r in range(nrows):
        assert redc(a, bs[r]) % p == u1 * z[r] * R32 % p and redc(a, bs[r]) + (p - 1) > 2 * p
    return shape, z, run, u1
