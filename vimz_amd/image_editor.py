"""Input tooling: image -> packed rows -> VIMz input JSON.

Host-side mirror of the reference's Python input generator (pyvimz/pyvimz/image_editor.py:71-150,
pyvimz/pyvimz/img/ops.py:4-105, pyvimz/pyvimz/img/transformations.py:6-147), restated with integer
numpy arithmetic so that it is bit-exact against the reference's outputs (pinned in
tests/test_oracle_golden.py against the reference's committed PNGs/hashes and against fixtures minted
by importing pyvimz, see tests/golden/make_fixtures.py).

Packing (ops.py:17-31, circuits/src/utils/pixels.circom:15-27): 10 pixels per field element, pixel k
in bits [24k, 24k+24), R in the low byte — i.e. the 30 little-endian bytes of an element are exactly
the raw R,G,B bytes of its 10 pixels.  Grayscale: the value sits in the low byte of each 24-bit slot.
Rows are returned as uint64 limb arrays of shape (rows, width, 4) (canonical little-endian), the
layout the C ABI (include/vimz_hip.h) takes; `rows_to_hex` renders the reference's "0x…" strings.

The functions below are the specification.  gpu_edit, gpu_build_input and gpu_edit_chain compute the same bytes on the GPU
(vimz_image_edit, vimz_amd/csrc/image_edit.hip); they have no CPU path.  The command line is the GPU editor, as pyvimz's `image-editor`:

    python -m vimz_amd.image_editor OPERATION -i IMAGE [-o OUT] [--save-png PNG] [--factor F] [--x X --y Y --crop-size SD|HD|FHD]
                                    [--resize-option "HD to SD"|"4K to FHD"] [--redact-flags FILE] [--device D]
"""
import argparse
import json
import os
import sys

import numpy as np

PACKING_FACTOR = 10  # vimz/src/lib.rs:10


def compress_by_rows(image):
    """image: (H, W, 3) or (H, W) uint8 -> (H, ceil(W/10), 4) uint64 limbs (ops.py:4-33)."""
    img = np.asarray(image, dtype=np.uint8)
    h, w = img.shape[:2]
    n = (w + PACKING_FACTOR - 1) // PACKING_FACTOR
    buf = np.zeros((h, n * PACKING_FACTOR, 3), dtype=np.uint8)
    if img.ndim == 2:
        buf[:, :w, 0] = img
    else:
        buf[:, :w, :] = img[:, :, :3]
    out = np.zeros((h, n, 32), dtype=np.uint8)
    out[:, :, :30] = buf.reshape(h, n, 30)
    return out.view("<u8").reshape(h, n, 4)


def compress_by_blocks(image, block=40):
    """(H, W[,3]) -> (blocks, block*block/10, 4) limbs, blocks row-major (ops.py:36-70)."""
    img = np.asarray(image, dtype=np.uint8)
    h, w = img.shape[:2]
    blocks = []
    for br in range(0, h, block):
        for bc in range(0, w, block):
            sub = img[br:br + block, bc:bc + block]
            blocks.append(compress_by_rows(sub).reshape(-1, 4))
    return np.stack(blocks)


def rows_to_hex(rows):
    """(R, W, 4) limbs -> list of list of '0x…' strings, formatted as the reference does (ops.py:21-27)."""
    rows = np.asarray(rows, dtype=np.uint64)
    out = []
    for r in rows:
        line = []
        for e in r:
            v = int(e[0]) | int(e[1]) << 64 | int(e[2]) << 128 | int(e[3]) << 192
            line.append("0x" + format(v, "060x"))
        out.append(line)
    return out


def hex_to_rows(rows_hex):
    """list of list of hex strings -> (R, W, 4) limbs (vimz/src/input.rs:95-105)."""
    R = len(rows_hex)
    W = len(rows_hex[0]) if R else 0
    out = np.zeros((R, W, 4), dtype=np.uint64)
    for i, r in enumerate(rows_hex):
        for j, s in enumerate(r):
            v = int(s, 16)
            for k in range(4):
                out[i, j, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


# ---------------------------------------------------------------- transformations (integer restatements)

def convert_to_grayscale(img):
    """Pillow's 'L' conversion (transformations.py:40-41): (19595 R + 38470 G + 7471 B + 32768) >> 16."""
    a = np.asarray(img, dtype=np.uint32)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 32768) >> 16).astype(np.uint8)


def adjust_contrast(img, factor):
    """transformations.py:44-56, same float64 expression: ((c - 128.0) * f + 128.0).clip(0, 255) truncated to uint8.
    (Equals clip((c-128)*f10 + 1280, 0, 2550) // 10 on the reference's samples; the float form is kept so every
    factor rounds exactly as the reference does.)"""
    a = np.asarray(img)[..., :3].astype(np.float64)
    mean = float(int(128 * 1000)) / 1000
    return ((a - mean) * factor + mean).clip(0, 255).astype(np.uint8)


def adjust_brightness(img, factor):
    """transformations.py:59-63: clip(float(c) * f, 0, 255) truncated to uint8 (float64, as the reference)."""
    a = np.asarray(img)[..., :3].astype(float)
    return np.clip(a * factor, 0, 255).astype(np.uint8)


def _conv3(chan, kernel, weight):
    """ops.py:73-105 conv2d with zero padding, floor division, clamp to [0,255]."""
    h, w = chan.shape
    p = np.zeros((h + 2, w + 2), dtype=np.int64)
    p[1:-1, 1:-1] = chan
    acc = np.zeros((h, w), dtype=np.int64)
    for m in range(3):
        for n in range(3):
            if kernel[m][n]:
                acc += kernel[m][n] * p[m:m + h, n:n + w]
    return np.clip(acc // weight, 0, 255).astype(np.uint8)


def blur_image(img):
    a = np.asarray(img, dtype=np.int64)[..., :3]
    k = [[1, 1, 1], [1, 1, 1], [1, 1, 1]]
    return np.dstack([_conv3(a[..., c], k, 9) for c in range(3)])


def sharpen_image(img):
    a = np.asarray(img, dtype=np.int64)[..., :3]
    k = [[0, -1, 0], [-1, 5, -1], [0, -1, 0]]
    return np.dstack([_conv3(a[..., c], k, 1) for c in range(3)])


def crop_image(img, x, y, new_w, new_h):
    return np.asarray(img)[y:y + new_h, x:x + new_w]


def resize_image(img, new_h, new_w):
    """transformations.py:97-147.  HD->SD: rows 3->2 with weights (2/3,1/3)/(1/3,2/3), result/2 truncated to uint8;
    otherwise 2x2 box with weight 1/2 then /2.  The reference computes in float64; a*w+b*w+c*(1-w)+d*(1-w) is
    reproduced with the same float expression so the truncation matches exactly."""
    a = np.asarray(img)[..., :3].astype(np.float64)
    h, w, _ = a.shape
    xr, yr = float(w) / float(new_w), float(h) / float(new_h)
    ii = np.arange(new_h); jj = np.arange(new_w)
    yl = (ii * yr).astype(np.int64); xl = (jj * xr).astype(np.int64)
    A = a[yl][:, xl]; B = a[yl][:, xl + 1]; Cc = a[yl + 1][:, xl]; D = a[yl + 1][:, xl + 1]
    if h == 720:
        wt = np.where(ii % 2 == 0, 2.0, 1.0) / 3
        wt = wt[:, None, None]
        summ = A * wt + B * wt + Cc * (1 - wt) + D * (1 - wt)
    else:
        wt = 0.5
        summ = A * wt + B * wt + Cc * wt + D * wt
    return (summ / 2).astype(np.uint8)


def random_image_redaction(img, block=40):
    """Checkerboard redaction (transformations.py:71-94): block (by,bx) is zeroed when by+bx is odd."""
    a = np.array(img)
    h, w = a.shape[:2]
    ind = []
    out = a.copy()
    for by in range(h // block):
        for bx in range(w // block):
            red = (by + bx) % 2 == 1
            ind.append(1 if red else 0)
            if red:
                out[by * block:(by + 1) * block, bx * block:(bx + 1) * block] = 0
    return out, ind


SIZE_MAP = {"sd": (640, 480), "hd": (1280, 720), "fhd": (1920, 1080)}


def build_input(operation, image, factor=None, x=None, y=None, crop_size=None, resize_to=None):
    """Mirror of image_editor.main (image_editor.py:71-150): returns the VIMzInput as a dict of limb arrays
    {"original": (R,W,4), "transformed": (R',W',4) or None, "factor"|"info"|"redact": ...}."""
    img = np.asarray(image)[..., :3]
    out = {"original": compress_by_rows(img), "transformed": None}
    if operation == "hash":
        pass
    elif operation == "grayscale":
        out["transformed"] = compress_by_rows(convert_to_grayscale(img))
    elif operation in ("brightness", "contrast"):
        fn = adjust_brightness if operation == "brightness" else adjust_contrast
        out["transformed"] = compress_by_rows(fn(img, factor))
        out["factor"] = int(factor * 10)
    elif operation in ("sharpness", "blur"):
        fn = sharpen_image if operation == "sharpness" else blur_image
        zeros = np.zeros((1, out["original"].shape[1], 4), dtype=np.uint64)
        out["original"] = np.concatenate([zeros, out["original"], zeros])
        out["transformed"] = compress_by_rows(fn(img))
    elif operation == "crop":
        w, h = SIZE_MAP[crop_size.lower()]
        out["transformed"] = compress_by_rows(crop_image(img, x, y, w, h))
        out["info"] = x * 2 ** 24 + y * 2 ** 12
    elif operation == "redact":
        out["original"] = compress_by_blocks(img)
        tr, ind = random_image_redaction(img)
        out["redact"] = ind
        out["transformed"] = compress_by_blocks(tr)
    elif operation == "resize":
        w, h = resize_to
        out["transformed"] = compress_by_rows(resize_image(img, h, w))
    else:
        raise ValueError(f"unknown operation {operation}")
    return out


def dump_json(inp, path):
    """Write the reference's JSON schema (vimz/src/input.rs:9-62)."""
    d = {"original": rows_to_hex(inp["original"])}
    if inp.get("transformed") is not None:
        d["transformed"] = rows_to_hex(inp["transformed"])
    for k in ("factor", "info"):
        if k in inp:
            d[k] = int(inp[k])
    if "redact" in inp:
        d["redact"] = ["0x1" if r else "0x0" for r in inp["redact"]]
    with open(path, "w") as fp:
        json.dump(d, fp, indent=4)


def load_json(path):
    with open(path) as fp:
        d = json.load(fp)
    out = {"original": hex_to_rows(d["original"]), "transformed": hex_to_rows(d["transformed"]) if d.get("transformed") else None}
    for k in ("factor", "info"):
        if k in d:
            out[k] = int(d[k])
    if "redact" in d:
        out["redact"] = [int(s, 16) for s in d["redact"]]
    return out


# ---------------------------------------------------------------- the same edits on the GPU (vimz_image_edit)

OPERATIONS = ("blur", "brightness", "contrast", "crop", "grayscale", "hash", "redact", "resize", "sharpness")
RESIZE_OPTIONS = {"hd to sd": (640, 480), "4k to fhd": (1920, 1080)}      # pyvimz image_editor.py's --resize-option
BLOCK = 40


def _crop_wh(crop_size):
    if isinstance(crop_size, str):
        if crop_size.lower() not in SIZE_MAP:
            raise ValueError(f"crop size {crop_size!r}: one of SD, HD, FHD, or a (width, height) pair")
        return SIZE_MAP[crop_size.lower()]
    w, h = crop_size
    return int(w), int(h)


def _edit_desc(op, factor=None, x=None, y=None, crop_size=None, resize_to=None, redact=None):
    """The parameters of `op` as a hip.Context.image_edit descriptor (without its source)."""
    if op not in OPERATIONS:
        raise ValueError(f"unknown operation {op!r}")
    d = {"op": op}
    if op in ("brightness", "contrast"):
        if factor is None:
            raise ValueError(f"{op} needs a factor")
        d["factor"] = float(factor)
    elif op == "crop":
        if x is None or y is None or crop_size is None:
            raise ValueError("crop needs x, y and crop_size")
        w, h = _crop_wh(crop_size)
        d.update(x=int(x), y=int(y), new_width=w, new_height=h)
    elif op == "resize":
        if resize_to is None:
            raise ValueError("resize needs resize_to = (width, height)")
        w, h = resize_to
        d.update(new_width=int(w), new_height=int(h))
    elif op == "redact" and redact is not None:
        d["redact"] = np.asarray(redact).reshape(-1)
    return d


def _input_fields(op, params, shape):
    """build_input's scalar fields of `op` for a source of `shape`: factor, info, or the redact flags (pyvimz's checkerboard by default)."""
    out = {}
    if op in ("brightness", "contrast"):
        out["factor"] = int(params["factor"] * 10)
    elif op == "crop":
        out["info"] = params["x"] * 2 ** 24 + params["y"] * 2 ** 12
    elif op == "redact":
        if params.get("redact") is not None:
            out["redact"] = [1 if v else 0 for v in np.asarray(params["redact"]).reshape(-1)]
        else:
            out["redact"] = [(by + bx) % 2 for by in range(shape[0] // BLOCK) for bx in range(shape[1] // BLOCK)]
    return out


def _source(image):
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise ValueError(f"an image is uint8, not {img.dtype}")
    return img


def _run(ctx, descs):
    if ctx is not None:
        return ctx.image_edit(descs)
    from .hip import Context
    with Context(0) as c:
        return c.image_edit(descs)


def _as_input(op, params, shape, res):
    inp = {"original": res["source"], "transformed": res["target"]}
    inp.update(_input_fields(op, params, shape))
    return inp


def gpu_edit(ctx, op, image, **params):
    """The edited image of `op` on the GPU: the bytes the host function above returns for image[..., :3] (redact: its image, not its flags).
    params: factor (brightness, contrast), x, y, crop_size ("SD" / "HD" / "FHD" or (width, height)), resize_to ((width, height)), redact (one
    flag per full 40 x 40 block, row-major; default pyvimz's checkerboard).  ctx: a hip.Context, or None for a context on device 0."""
    d = _edit_desc(op, **params)
    d.update(pixels=_source(image), want=("pixels",))
    return _run(ctx, [d])[0]["pixels"]


def gpu_build_input(ctx, op, image, factor=None, x=None, y=None, crop_size=None, resize_to=None, redact=None):
    """build_input on the GPU: the same arrays and fields.  redact= takes the caller's flags (one per full 40 x 40 block, row-major), which
    build_input cannot; the input's "redact" field then holds them."""
    params = {"factor": factor, "x": x, "y": y, "crop_size": crop_size, "resize_to": resize_to, "redact": redact}
    img = _source(image)
    d = _edit_desc(op, **params)
    d.update(pixels=img, want=("source", "target"))
    return _as_input(op, params, img.shape, _run(ctx, [d])[0])


def gpu_edit_chain(ctx, image, stages):
    """Several edits in ONE call, each on the previous one's result (kept on the device): stages = [(op, params), ...], e.g.
    [("sharpness", {}), ("grayscale", {})].  Returns one (edited image, build_input dict of that stage) per stage."""
    img = _source(image)
    descs = []
    for i, (op, params) in enumerate(stages):
        d = _edit_desc(op, **dict(params))
        if i == 0:
            d["pixels"] = img
        else:
            d["source"] = i - 1
        descs.append(d)
    if not descs:
        return []
    res = _run(ctx, descs)
    out, shape = [], img.shape
    for (op, params), r in zip(stages, res):
        p = {"factor": None, "x": None, "y": None, "redact": None}
        p.update(params)
        out.append((r["pixels"], _as_input(op, p, shape, r)))
        shape = r["pixels"].shape
    return out


def _load(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGB")
        return np.array(im)


def _read_flags(path):
    """--redact-flags: a JSON list of 0 / 1 (or the input JSON's "0x0" / "0x1" strings), or whitespace-separated 0 / 1."""
    with open(path) as fp:
        text = fp.read()
    try:
        vals = json.loads(text)
    except ValueError:
        vals = text.split()
    if isinstance(vals, dict):
        vals = vals.get("redact")
    if not isinstance(vals, list):
        raise ValueError(f"{path}: not a list of flags")
    return [int(v, 0) if isinstance(v, str) else int(v) for v in vals]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vimz_amd.image_editor",
                                 description="Edit an image on the GPU and write the prover's input JSON (pyvimz's image-editor).")
    ap.add_argument("operation", choices=OPERATIONS)
    ap.add_argument("--image-path", "-i", required=True, help="the source image")
    ap.add_argument("--output", "-o", default="./", help="a file, or a directory for <operation>.json (default: the current directory)")
    ap.add_argument("--save-png", help="also save the edited image as a PNG")
    ap.add_argument("--factor", type=float, help="brightness, contrast")
    ap.add_argument("--x", type=int, help="crop: the window's left column")
    ap.add_argument("--y", type=int, help="crop: the window's top row")
    ap.add_argument("--crop-size", choices=["SD", "HD", "FHD"])
    ap.add_argument("--resize-option", choices=["HD to SD", "4K to FHD"])
    ap.add_argument("--redact-flags", help="redact: a file of flags, one per full 40 x 40 block, row-major (default: pyvimz's checkerboard)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    op = a.operation
    if op in ("brightness", "contrast") and a.factor is None:
        ap.error(f"{op} needs --factor")
    if op == "crop" and (a.x is None or a.y is None or a.crop_size is None):
        ap.error("crop needs --x, --y and --crop-size")
    if op == "resize" and a.resize_option is None:
        ap.error("resize needs --resize-option")
    if a.redact_flags is not None and op != "redact":
        ap.error("--redact-flags is for redact only")
    try:
        flags = _read_flags(a.redact_flags) if a.redact_flags else None
        img = _load(a.image_path)
    except (OSError, ValueError) as e:
        print(f"image_editor: {e}", file=sys.stderr)
        return 1
    params = {"factor": a.factor, "x": a.x, "y": a.y, "crop_size": a.crop_size, "redact": flags,
              "resize_to": RESIZE_OPTIONS[a.resize_option.lower()] if a.resize_option else None}
    from . import _lib, hip
    try:
        with hip.Context(a.device) as ctx:
            d = _edit_desc(op, **params)
            d["pixels"] = img
            res = ctx.image_edit([d])[0]
    except (_lib.VimzError, ValueError) as e:
        print(f"image_editor: {e}", file=sys.stderr)
        return 1
    out = os.path.join(a.output, f"{op}.json") if os.path.isdir(a.output) else a.output
    dump_json(_as_input(op, params, img.shape, res), out)
    print(f"Transformation {op} applied successfully. Data saved to {out}.")
    if a.save_png and op != "hash":
        from PIL import Image
        Image.fromarray(res["pixels"]).save(a.save_png)
        print(f"Transformed image saved as {a.save_png}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
