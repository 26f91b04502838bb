"""Edge inputs for the witness generator (vimz_amd/csrc/witness.hpp), built without a GPU and without library state.

`cases()` returns {circuit key: (Circuit arguments, [Run, ...])}.  A Run is (z0, rows, expect, name): the IVC state the run
starts from, its rows' private inputs as (n_priv, 4) limb arrays, and what the step relation says about them:
  "sat"                 every row satisfies the relation;
  a tuple, one per row  "sat", "unsat" (the relation has no solution: the executor flags the row or its wires violate the R1CS),
                        or "r1cs" (unsat, and the way it shows is fixed: the executor's status is 0 and its wires violate the R1CS —
                        crop's literal Decoder with x past the row).
Rows of one run are chained: row i starts from the state row i-1 left, satisfied or not (the hashes are computed either way).

The shapes are small on purpose: width 16 gives 160 or 480 lanes (2.5 or 7.5 blocks of 64 threads), width 9 gives 90 or 270 and an
array hash that ends in a three-wide permutation as HD's does; crop (16, 8, 3) has 83 lane groups with lane counts 1..160.

Targets come from the host editor (vimz_amd/image_editor.py), the specification; resize targets from the integer relation's exact
value (the editor's 3->2 branch wants 720 rows).  Expectations that are not plain "the editor's output satisfies" are derived here
from the relations' integer arithmetic (oracle/steps.hpp restates them), never from a run of the code under test:
  * contrast / brightness: LessEqThan(13)(adj, -adj) decomposes 2 adj + 8191 into 14 bits, so a row is satisfiable only while
    -4095 <= adj <= 4096 for all its pixels: (255 - 128) f + 1280 <= 4096 up to f = 22, 255 f <= 4096 up to f = 16;
  * tolerances: |value - k t| <= k with value an exact multiple of k, so t0 +- 1 satisfies and t0 +- 2 does not.  Uniform rows of
    v: v = 1 / 2 for the downward and 254 / 253 for the upward tampers where the relation allows it; blur needs its border value
    6 v to be a multiple of 9 (v = 3, 252), sharpness its border value 2 v to stay below 255 (v = 126)."""
from collections import namedtuple

import numpy as np

from vimz_amd import image_editor as ie

P_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
ROWS = 6
IMAGES = ("ones", "zeros", "checker", "stripes_v", "stripes_h", "random", "extremes")      # an all-255 image precedes the all-zero one
PIXEL_OPS = ("grayscale", "contrast", "brightness", "blur", "sharpness")
FACTOR10 = {"contrast": ((0, 1, 10, 14, 22), 23), "brightness": ((0, 1, 10, 16), 17)}      # satisfiable f10 values, the first that is not
DEFAULT_F10 = {"contrast": 14, "brightness": 12}
CROP_Y = 5

Run = namedtuple("Run", "z0 rows expect name")

CIRCUITS = {}
for _op in PIXEL_OPS:
    for _w in (16, 9):
        CIRCUITS[f"{_op}-{_w}"] = (_op, _w, 0, 0, 0, 0)
for _w in (8, 9, 16):
    CIRCUITS[f"hash-{_w}"] = ("hash", _w, 0, 0, 0, 0)
CIRCUITS["resize-3to2"] = ("resize", 16, 8, 3, 2, 0)
CIRCUITS["resize-2to1"] = ("resize", 16, 8, 2, 1, 0)
CIRCUITS["redact-16"] = ("redact", 16, 0, 0, 0, 0)
CIRCUITS["crop-16"] = ("crop", 16, 8, 0, 0, 3)
# shapes the builder accepts and the GPU prover refuses: their window-fold hasher needs a Poseidon width other than 3 or 9
REFUSED = {"hash-13": ("hash", 13, 0, 0, 0, 0), "crop-4-2": ("crop", 4, 2, 0, 0, 3)}


def step_kwargs(args):
    """oracle.step_eval's shape arguments of a circuit."""
    _, w, w2, ri, ro, ch = args
    return dict(width=w, width2=w2, rows_in=ri, rows_out=ro, crop_h=ch)


def expect_of(run, i):
    return run.expect if isinstance(run.expect, str) else run.expect[i]


def image(name, width):
    """(6, 10 width, 3) uint8."""
    W = 10 * width
    y, x = np.mgrid[0:ROWS, 0:W]
    rng = np.random.default_rng(1000 + IMAGES.index(name))
    if name == "zeros":
        g = np.zeros((ROWS, W), dtype=np.uint8)
    elif name == "ones":
        g = np.full((ROWS, W), 255, dtype=np.uint8)
    elif name == "checker":
        g = (((x + y) % 2) * 255).astype(np.uint8)
    elif name == "stripes_v":
        g = ((x % 2) * 255).astype(np.uint8)
    elif name == "stripes_h":
        g = ((y % 2) * 255).astype(np.uint8)
    elif name == "random":
        return rng.integers(0, 256, size=(ROWS, W, 3), dtype=np.uint8)
    elif name == "extremes":
        return rng.choice(np.array([0, 1, 127, 128, 129, 254, 255], dtype=np.uint8), size=(ROWS, W, 3))
    else:
        raise ValueError(name)
    return np.repeat(g[:, :, None], 3, axis=2)


def uniform(rows, width, v):
    return np.full((rows, 10 * width, 3), v, dtype=np.uint8)


def _elem(value):
    return np.array([[(value >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]], dtype=np.uint64)


def _set_bit(rows_limbs, elem, bit):
    out = rows_limbs.copy()
    out[elem, bit // 64] |= np.uint64(1 << (bit % 64))
    return out


def _add_to_pixel(row_limbs, x, colour, delta):
    """The packed row with byte (pixel x, colour) changed by delta; the byte must stay inside 0..255."""
    out = row_limbs.copy()
    b = out[x // 10].view(np.uint8)
    k = (x % 10) * 3 + colour
    v = int(b[k]) + delta
    assert 0 <= v <= 255, (x, colour, int(b[k]), delta)
    b[k] = v
    return out


# ---- targets -----------------------------------------------------------------------------------------------------------------------
def resize_exact(img, rows_in, rows_out):
    """The integer relation's exact value (oracle/steps.hpp T_RESIZE), rounded down: 3->2 (a wt + b (3 - wt)) // 6, 2->1 (a + b) // 4."""
    a = img.astype(np.int64)
    pair = a[:, 0::2] + a[:, 1::2]
    out = []
    for s in range(a.shape[0] // rows_in):
        for i in range(rows_out):
            up, down = pair[rows_in * s + i], pair[rows_in * s + i + 1]
            if rows_in == 3:
                wt = 2 if i % 2 == 0 else 1
                out.append((up * wt + down * (3 - wt)) // 6)
            else:
                out.append((up + down) // 4)
    return np.stack(out).astype(np.uint8)


def target(op, img, f10=None):
    if op == "grayscale":
        return ie.convert_to_grayscale(img)
    if op == "contrast":
        return ie.adjust_contrast(img, f10 / 10)
    if op == "brightness":
        return ie.adjust_brightness(img, f10 / 10)
    if op == "blur":
        return ie.blur_image(img)
    if op == "sharpness":
        return ie.sharpen_image(img)
    raise ValueError(op)


def step_rows(op, img, tgt, rows_in=0, rows_out=0):
    """Per-step private inputs of an image and its target, in the reference's flattened order."""
    o, t = ie.compress_by_rows(img), ie.compress_by_rows(tgt)
    n = img.shape[0]
    if op in ("grayscale", "contrast", "brightness"):
        return [np.concatenate([o[i], t[i]]) for i in range(n)]
    if op in ("blur", "sharpness"):
        zero = np.zeros((1,) + o.shape[1:], dtype=np.uint64)
        pad = np.concatenate([zero, o, zero])
        return [np.concatenate([pad[i:i + 3].reshape(-1, 4), t[i]]) for i in range(n)]
    if op == "resize":
        return [np.concatenate([o[rows_in * s:rows_in * (s + 1)].reshape(-1, 4), t[rows_out * s:rows_out * (s + 1)].reshape(-1, 4)])
                for s in range(n // rows_in)]
    raise ValueError(op)


def z0_of(op, f10=None):
    if op in ("contrast", "brightness"):
        return [0, 0, f10]
    return {"grayscale": [0, 0], "blur": [0] * 4, "sharpness": [0] * 4, "resize": [0, 0]}[op]


def adjusted_in_range(op, row, f10):
    """Whether LessEqThan(13)(adj, -adj) has a solution for every pixel of the row: -4095 <= adj <= 4096."""
    a = row.astype(np.int64)
    adj = (a - 128) * f10 + 1280 if op == "contrast" else a * f10
    return bool(adj.min() >= -4095 and adj.max() <= 4096)


# ---- tolerance edges ---------------------------------------------------------------------------------------------------------------
def _tolerance_rows(op, width, args):
    """[(name, z0, row inputs, expect)] — one row each: uniform rows whose target is off by delta at one pixel of the last colour."""
    _, w, w2, rows_in, rows_out, _ = args
    out = []
    npix = 10 * (w2 if op == "resize" else width)
    colour = 0 if op == "grayscale" else 2
    for x in (0, 63, 64, npix - 1):
        for delta in (-1, 1, -2, 2):
            cands = range(1, 40) if delta < 0 else range(254, 100, -1)
            for v in cands:
                if op == "resize":
                    img = uniform(rows_in, width, v)
                    tgt = resize_exact(img, rows_in, rows_out)
                    rows = step_rows(op, img, tgt, rows_in, rows_out)[0]
                    t0, exact, trow = int(tgt[-1, x, colour]), True, len(rows) - w2
                elif op in ("blur", "sharpness"):
                    img = uniform(3, width, v)
                    tgt = target(op, img)
                    rows = step_rows(op, img, tgt)[1]      # the middle row's step: three uniform rows, zero padding left and right only
                    t0, trow = int(tgt[1, x, colour]), 3 * width
                    cols = 2 if x in (0, npix - 1) else 3
                    value = 3 * cols * v if op == "blur" else min(255, (5 - (cols - 1) - 2) * v)
                    exact = value == (9 if op == "blur" else 1) * t0
                else:
                    img = uniform(1, width, v)
                    tgt = target(op, img, 10)
                    rows = step_rows(op, img, tgt)[0]
                    t0, exact, trow = int(tgt[0, x] if op == "grayscale" else tgt[0, x, colour]), True, width
                    assert t0 == v
                if exact and 0 <= t0 + delta <= 255:
                    break
            else:
                raise AssertionError((op, x, delta))
            rows = rows.copy()
            rows[trow:] = _add_to_pixel(rows[trow:], x, colour, delta)
            out.append((f"tol-x{x}-{delta:+d}-v{v}", z0_of(op, 10), rows, "sat" if abs(delta) == 1 else "unsat"))
    return out


def _batched(prefix, items, per_run=8):
    """Rows that do not depend on each other's states, as runs of up to eight rows."""
    runs = []
    for k in range(0, len(items), per_run):
        part = items[k:k + per_run]
        runs.append(Run(part[0][1], [r for _, _, r, _ in part], tuple(e for _, _, _, e in part), f"{prefix}-{k // per_run}:" + ",".join(n for n, _, _, _ in part)))
    return runs


# ---- the runs of each circuit --------------------------------------------------------------------------------------------------------
def _pixel_runs(op, width, args):
    runs = []
    f_default = DEFAULT_F10.get(op)
    for name in IMAGES:
        img = image(name, width)
        runs.append(Run(z0_of(op, f_default), step_rows(op, img, target(op, img, f_default)), "sat", name))
    if op in FACTOR10:
        sat, first_unsat = FACTOR10[op]
        for name in ("extremes", "checker"):
            img = image(name, width)
            for f10 in sat + ((first_unsat,) if width == 16 else ()):
                exp = tuple("sat" if adjusted_in_range(op, img[i], f10) else "unsat" for i in range(ROWS))
                # the ceilings are pinned on every row: these images hold 0 and 254 or 255 in each row
                assert exp == (("sat",) * ROWS if f10 in sat else ("unsat",) * ROWS), (op, name, f10, exp)
                runs.append(Run(z0_of(op, f10), step_rows(op, img, target(op, img, f10)), "sat" if f10 in sat else exp, f"{name}-f{f10}"))
    tol = _tolerance_rows(op, width, args)
    if op in ("blur", "sharpness"):      # a row's state must follow from the rows before it: one run each, from the zero state
        runs += [Run(z, [r], (e,), n) for n, z, r, e in tol]
    else:
        runs += _batched("tol", tol)
    # range edges: bit 239 of a packed element is the top bit of its last byte (set in every element of the all-255 image, which is
    # among the runs above); bit 240 is past the decomposition
    img = image("ones", width)
    good = step_rows(op, img, target(op, img, f_default))[2]
    assert all((int(e[3]) >> (239 - 192)) & 1 for e in good[:width])
    rng = [("bit239", z0_of(op, f_default), good, "sat"),
           ("bit240-first", z0_of(op, f_default), _set_bit(good, 0, 240), "unsat"),
           ("bit240-last", z0_of(op, f_default), _set_bit(good, len(good) - 1, 240), "unsat")]
    if op in ("blur", "sharpness"):
        runs += [Run(z, [r], (e,), n) for n, z, r, e in rng]
    else:
        runs += _batched("range", rng)
    if op in FACTOR10 and width == 16:
        img = image("checker", width)
        rows = step_rows(op, img, target(op, img, 10))
        runs.append(Run([0, 0, 1 << 40], rows[:2], ("unsat", "unsat"), "factor-2^40"))               # LOP_LDZ's range
        runs.append(Run([0, 0, (1 << 40) - 1], rows[:2], ("unsat", "unsat"), "factor-2^40-1"))       # the lanes' bit decompositions
    if op == "contrast" and width == 16:
        # a failure in the middle of a batch: rows do not depend on each other beyond the hashes, which tampering does not break
        img = image("random", width)
        rows = step_rows(op, img, target(op, img, 10))[:5]
        t0 = int(rows[2][width:].view(np.uint8).reshape(-1, 32)[15, 29])
        rows[2] = rows[2].copy()
        rows[2][width:] = _add_to_pixel(rows[2][width:], 159, 2, 2 if t0 <= 253 else -2)
        # (at f10 = 10 the editor's target is the exact value, so two units leave the tolerance of one)
        runs.append(Run(z0_of(op, 10), rows, ("sat", "sat", "unsat", "sat", "sat"), "mid-batch"))
    return runs


def _hash_runs(width):
    runs = [Run([P_MOD - 1], list(ie.compress_by_rows(image("ones", width))), "sat", "ones-from-p-1")]
    for name in IMAGES[1:]:
        runs.append(Run([0], list(ie.compress_by_rows(image(name, width))), "sat", name))
    return runs


def _redact_runs(width):
    runs = []
    for k, name in enumerate(("ones", "zeros", "checker", "random", "extremes")):
        o = ie.compress_by_rows(image(name, width))
        rows = [np.concatenate([o[i], _elem((i + k) % 2)]) for i in range(ROWS)]
        runs.append(Run([P_MOD - 1, P_MOD - 2] if k == 0 else [0, 0], rows, "sat", f"{name}-flags{k % 2}"))
    return runs


def _resize_runs(args):
    op, width, w2, rows_in, rows_out, _ = args
    runs = []
    for name in IMAGES:
        img = image(name, width)
        runs.append(Run([0, 0], step_rows(op, img, resize_exact(img, rows_in, rows_out), rows_in, rows_out), "sat", name))
    runs += _batched("tol", _tolerance_rows(op, width, args))
    img = image("ones", width)
    good = step_rows(op, img, resize_exact(img, rows_in, rows_out), rows_in, rows_out)[0]
    runs += _batched("range", [("bit239", [0, 0], good, "sat"), ("bit240-first", [0, 0], _set_bit(good, 0, 240), "unsat"),
                               ("bit240-last", [0, 0], _set_bit(good, len(good) - 1, 240), "unsat")])
    return runs


def crop_info(row_index, y, x):
    return (row_index << 24) | (y << 12) | x


def _crop_runs(args):
    _, width, w2, _, _, height = args
    y = CROP_Y
    runs = []
    for name in ("ones", "zeros", "random"):
        runs.append(Run([0, 0, crop_info(y + 1, y, 0)], list(ie.compress_by_rows(image(name, width))), "sat", name))
    rnd = ie.compress_by_rows(image("random", width))
    for x in (0, 80, 81, 159):
        for k, ri in enumerate((y - 1, y, y + height - 1, y + height)):      # just outside and just inside the window, at both ends
            runs.append(Run([0, 0, crop_info(ri, y, x)], [rnd[k]], "sat", f"x{x}-row{ri}"))
    for x in (160, 4095):      # the literal Decoder: no status, a witness that violates the R1CS
        runs.append(Run([0, 0, crop_info(y, y, x)], [rnd[0]], ("r1cs",), f"x{x}"))
    runs.append(Run([3, 4, crop_info(y, y, 79)], [rnd[0], rnd[1], rnd[2]], "sat", "three-rows"))      # info + 1 chains
    ones = ie.compress_by_rows(image("ones", width))[0]
    runs.append(Run([0, 0, crop_info(y, y, 0)], [_set_bit(ones, 0, 240)], ("unsat",), "bit240"))
    runs.append(Run([0, 0, crop_info(y, y, 0)], [_set_bit(image_row_zero(width), width - 1, 239)], "sat", "bit239"))
    return runs


def image_row_zero(width):
    return ie.compress_by_rows(image("zeros", width))[0]


_cache = None


def cases():
    """{key: (Circuit arguments, [Run])}, built once."""
    global _cache
    if _cache is None:
        out = {}
        for key, args in CIRCUITS.items():
            op, width = args[0], args[1]
            if op in PIXEL_OPS:
                runs = _pixel_runs(op, width, args)
            elif op == "hash":
                runs = _hash_runs(width)
            elif op == "redact":
                runs = _redact_runs(width)
            elif op == "resize":
                runs = _resize_runs(args)
            else:
                runs = _crop_runs(args)
            names = [r.name for r in runs]
            assert len(set(names)) == len(names), key
            out[key] = (args, runs)
        _cache = out
    return _cache


def find(key, name):
    for r in cases()[key][1]:
        if r.name == name:
            return r
    raise KeyError((key, name))


def n_triples():
    """The number of (circuit, run, row) triples."""
    return sum(len(r.rows) for _, runs in cases().values() for r in runs)
