"""Image hashes on the GPU: the running Poseidon hash the circuits keep of an image (vimz_image_hash, include/vimz_hip.h).

The value pyvimz's `image-hasher` computes (pyvimz/pyvimz/image_hasher.py, one circom witness-generator process per row) and writes to
marketplace/image-data/*.hash, and what a proof's final state holds in z_n[0] (source) and z_n[1] (target):

    units   rows packed 10 pixels per element (compress_by_rows), or 40 x 40 blocks (compress_by_blocks: redact)
    digest  d_i = ArrayHasher(L)(unit i)
    hash    acc_0 = 0, acc_{i+1} = PairHasher(acc_i, d_i)   (PairHasher(acc_i, 0) for a dropped unit: a redacted block)

Command line, as pyvimz's `image-hasher <image_path> [<output_path>]`:

    python -m vimz_amd.image_hasher IMAGE [OUT] [--rows N] [--blocks] [--device D]

prints the decimal hash and writes it to OUT as the .hash files hold it (no newline).  There is no CPU path: without a GPU it fails.
"""
import argparse
import os
import sys

import numpy as np

from . import _lib

BLOCK = 40      # the redact circuit's block side (compress_by_blocks)


def load_image(image):
    """A path (opened with PIL as pyvimz does: np.array(Image.open(path))) or an array, as a uint8 (H, W) / (H, W, C) array."""
    if isinstance(image, (str, bytes, os.PathLike)):
        from PIL import Image
        with Image.open(image) as im:
            image = np.array(im)
    return np.asarray(image)


def _spec(item):
    if isinstance(item, dict):
        return dict(item)
    return {"image": item}


def _desc(spec):
    """One hashing request {image, mode="rows"|"blocks", units=None, drop=None} -> a descriptor for hip.Context.image_hash."""
    mode = spec.get("mode", "rows")
    if mode not in ("rows", "blocks"):
        raise ValueError(f"mode must be 'rows' or 'blocks', not {mode!r}")
    img = load_image(spec["image"])
    if img.dtype == np.uint64:        # pre-packed canonical elements (U, L, 4)
        if img.ndim != 3 or img.shape[2] != 4 or mode != "rows":
            raise ValueError("pre-packed units are a (units, length, 4) uint64 array, hashed unit by unit (mode 'rows')")
        d = {"units": img}
        total = img.shape[0]
    else:
        if img.dtype != np.uint8:
            raise ValueError(f"an image is uint8, not {img.dtype}")
        if img.ndim == 3 and img.shape[2] == 1:
            img = img[:, :, 0]
        if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (3, 4)) or 0 in img.shape:
            raise ValueError(f"an image is (H, W) grey, (H, W, 3) RGB or (H, W, 4) RGBA, not {img.shape}")
        block = BLOCK if mode == "blocks" else 0
        d = {"pixels": img, "block": block}
        h, w = img.shape[:2]
        total = -(-h // block) * -(-w // block) if block else h
    units = spec.get("units")
    n = total if units is None else int(units)
    if not 1 <= n <= total:
        raise ValueError(f"{n} units asked for, the image has {total} {'blocks' if mode == 'blocks' else 'rows'}")
    d["max_units"] = n
    if spec.get("drop") is not None:
        drop = np.asarray(spec["drop"]).reshape(-1)
        if drop.size < n:
            raise ValueError(f"{drop.size} drop flags for {n} units")
        d["drop"] = (drop[:n] != 0).astype(np.uint8)
    return d


def image_hashes(ctx, items):
    """The hashes of several images in ONE call (one kernel launch for all their units; the host chains side by side).
    items: images (arrays or paths) or dicts {image, mode, units, drop} as image_hash takes them.  Returns a list of ints."""
    descs = [_desc(_spec(x)) for x in items]
    if not descs:
        return []
    return ctx.image_hash(descs)


def image_hash(ctx, image, mode="rows", units=None, drop=None):
    """The running hash of one image.  mode "rows" (every transformation but redact) or "blocks" (40 x 40 blocks: redact); units: hash only the
    first `units` rows / blocks (a demo proof covers DEMO_STEPS of them); drop: one flag per hashed unit, set for a redacted block."""
    return image_hashes(ctx, [{"image": image, "mode": mode, "units": units, "drop": drop}])[0]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vimz_amd.image_hasher", description="Running Poseidon hash of an image, on the GPU (pyvimz's image-hasher).")
    ap.add_argument("image")
    ap.add_argument("output", nargs="?", help="write the decimal hash here, without a newline (the format of marketplace/image-data/*.hash)")
    ap.add_argument("--rows", type=int, default=None, help="hash only the first N rows (blocks with --blocks)")
    ap.add_argument("--blocks", action="store_true", help="40 x 40 blocks instead of rows (the redact circuit's units)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from . import hip
    try:
        with hip.Context(a.device) as ctx:
            h = image_hash(ctx, a.image, mode="blocks" if a.blocks else "rows", units=a.rows)
    except (_lib.VimzError, ValueError, OSError) as e:
        print(f"image_hasher: {e}", file=sys.stderr)
        return 1
    s = str(h)
    print(s)
    if a.output:
        with open(a.output, "w") as fp:
            fp.write(s)
    return 0


if __name__ == "__main__":
    sys.exit(main())
