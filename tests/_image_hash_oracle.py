"""The running image hash on the CPU oracle — TEST INFRASTRUCTURE ONLY (the image-hash tests, and tools/image_hash_bench.py's host baseline).

A hasher for vimz_amd.folding.expected_final_state / verify_final_state (`hasher=`): it takes the request dicts of vimz_amd.image_hasher.image_hashes
({image, mode, units, drop}) and returns the hashes, computed with the oracle's ArrayHasher (orc_array_hash) per unit and its Poseidon for the chain."""
import ctypes as C
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests._oracle import from_limbs
from vimz_amd import image_editor as ie
from vimz_amd import image_hasher


def packed_units(spec):
    """(units (U, L, 4) uint64, drop flags or None) of one request, packed by the host image editor (compress_by_rows / compress_by_blocks)."""
    img = image_hasher.load_image(spec["image"])
    if img.dtype == np.uint64:
        rows = img
    elif spec.get("mode", "rows") == "blocks":
        rows = ie.compress_by_blocks(img)
    else:
        rows = ie.compress_by_rows(img)
    n = spec.get("units") or len(rows)
    assert 1 <= n <= len(rows), (n, len(rows))
    drop = spec.get("drop")
    return np.ascontiguousarray(rows[:n], dtype=np.uint64), (None if drop is None else [int(v) for v in list(drop)[:n]])


def digests(orc, units, drop=None, pool=None):
    """ArrayHasher(L) of every unit (0 for a dropped one), optionally over a thread pool (ctypes releases the GIL)."""
    L = units.shape[1]

    def one(u):
        if drop is not None and drop[u]:
            return 0
        o = np.zeros(4, dtype=np.uint64)
        orc.lib.orc_array_hash(C.c_void_p(units[u].ctypes.data), L, C.c_void_p(o.ctypes.data))
        return from_limbs(o)[0]
    return list(pool.map(one, range(len(units)))) if pool is not None else [one(u) for u in range(len(units))]


def chain(orc, ds):
    acc = 0
    for d in ds:
        acc = orc.poseidon([acc, d])
    return acc


def image_hash(orc, spec, pool=None):
    units, drop = packed_units(spec)
    return chain(orc, digests(orc, units, drop, pool))


def hasher(orc, threads=8):
    """A `hasher=` for vimz_amd.folding: the oracle's hashes, memoised per (pixels, mode, units, drop) so that a test module hashes each image once.
    hasher.calls records every request list it was given."""
    memo = {}
    pool = ThreadPoolExecutor(threads) if threads > 1 else None

    def run(specs):
        run.calls.append(list(specs))
        out = []
        for s in specs:
            img = np.ascontiguousarray(image_hasher.load_image(s["image"]))
            drop = s.get("drop")
            key = (hashlib.sha1(img.tobytes()).hexdigest(), img.shape, str(img.dtype), s.get("mode", "rows"), s.get("units"),
                   None if drop is None else tuple(int(v) for v in drop))
            if key not in memo:
                memo[key] = image_hash(orc, dict(s, image=img), pool)
            out.append(memo[key])
        return out
    run.calls = []
    return run
