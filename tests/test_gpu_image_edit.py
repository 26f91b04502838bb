"""vimz_image_edit on the MI355X: every transformation byte for byte against the host editor (vimz_amd/image_editor.py, the specification),
its float64 rounding over every factor k/1000, the reference's image hashes and pyvimz-minted rows, chains in one call, folded proofs built
from its inputs, and its refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _data
from vimz_amd import _lib, folding, hip, image_hasher
from vimz_amd import image_editor as ie

pytestmark = pytest.mark.gpu

KAT = _data.kat()
OPS = ie.OPERATIONS


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _upscaled(k):
    """img2 upscaled by nearest neighbour, as tests/_data.config_rows builds the 4K (k = 3) and 8K (k = 6) images."""
    img = _data.load_image("img2")
    return np.ascontiguousarray(np.repeat(np.repeat(img, k, axis=0), k, axis=1))


def _params(op, img):
    h, w = img.shape[:2]
    if op in ("contrast", "brightness"):
        return {"factor": 1.4}
    if op == "crop":
        if h >= 1180 and w >= 2120:
            return {"x": 200, "y": 100, "crop_size": "FHD"}
        if h >= 580 and w >= 840:
            return {"x": 200, "y": 100, "crop_size": "SD"}
        return {"x": w // 3, "y": h // 3, "crop_size": (w // 2, h // 2)}
    if op == "resize":
        return {"resize_to": (640, 480)} if h == 720 else {"resize_to": (w // 2, h // 2)}
    return {}


def _host_edit(op, img, p):
    img = img[..., :3] if img.ndim == 3 else img
    if op == "hash":
        return img
    if op == "grayscale":
        return ie.convert_to_grayscale(img)
    if op == "contrast":
        return ie.adjust_contrast(img, p["factor"])
    if op == "brightness":
        return ie.adjust_brightness(img, p["factor"])
    if op == "blur":
        return ie.blur_image(img)
    if op == "sharpness":
        return ie.sharpen_image(img)
    if op == "crop":
        w, h = ie._crop_wh(p["crop_size"])
        return ie.crop_image(img, p["x"], p["y"], w, h)
    if op == "resize":
        w, h = p["resize_to"]
        return ie.resize_image(img, h, w)
    return ie.random_image_redaction(img)[0]


def _assert_input_equal(got, want, what):
    assert np.array_equal(got["original"], want["original"]), (what, "original")
    if want["transformed"] is None:
        assert got["transformed"] is None, what
    else:
        assert np.array_equal(got["transformed"], want["transformed"]), (what, "transformed")
    for k in ("factor", "info", "redact"):
        assert (k in got) == (k in want) and got.get(k) == want.get(k), (what, k)


def _check_image(ctx, name, img):
    blocks = img.shape[0] % 40 == 0 and img.shape[1] % 40 == 0
    for op in OPS:
        p = _params(op, img)
        d = ie._edit_desc(op, **p)
        d["pixels"] = img
        if op == "redact" and not blocks:
            d["want"] = ("pixels",)
        res = ctx.image_edit([d])[0]
        assert np.array_equal(res["pixels"], _host_edit(op, img, p)), (name, op)
        if op == "redact" and not blocks:
            with pytest.raises(_lib.VimzError) as e:           # (build_input cannot pack blocks of this image either)
                ie.gpu_build_input(ctx, op, img, **p)
            assert e.value.code == _lib.ERR_INVALID
            continue
        got = ie._as_input(op, p, img.shape, res)
        if isinstance(p.get("crop_size", ""), str):
            _assert_input_equal(got, ie.build_input(op, img, **p), (name, op))
        else:                                                   # (build_input takes named crop sizes only)
            assert np.array_equal(got["original"], ie.compress_by_rows(img[..., :3])), (name, op)
            assert np.array_equal(got["transformed"], ie.compress_by_rows(res["pixels"])), (name, op)
            assert got["info"] == p["x"] * 2 ** 24 + p["y"] * 2 ** 12


@pytest.mark.parametrize("name", ["img1", "img2"])
def test_every_op_matches_the_host_editor_hd(ctx, name):
    _check_image(ctx, name, _data.load_image(name))


@pytest.mark.parametrize("resolution,k", [("4K", 3), ("8K", 6)])
def test_every_op_matches_the_host_editor_4k_8k(ctx, resolution, k):
    img = _upscaled(k)
    assert img.shape[:2] == {"4K": (2160, 3840), "8K": (4320, 7680)}[resolution]
    _check_image(ctx, resolution, img)


@pytest.mark.parametrize("shape", [(240, 320, 3), (41, 37, 3), (721, 1283, 3), (80, 95, 4), (57, 83, 1)])
def test_every_op_matches_the_host_editor_random_and_odd_sizes(ctx, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if shape[2] == 1:           # grey: the ops that take it
        img = img[:, :, 0]
        for op in ("hash", "crop", "redact"):
            p = _params(op, img)
            assert np.array_equal(ie.gpu_edit(ctx, op, img, **p), _host_edit(op, img, p)), op
        assert np.array_equal(ie.gpu_build_input(ctx, "hash", img)["original"], ie.compress_by_rows(img))
        return
    _check_image(ctx, str(shape), img)


def test_float64_rounding_every_factor(ctx):
    """A 256-value ramp in every channel through contrast and brightness at every factor k/1000, 0 <= k <= 3000, and a few non-decimal
    doubles: numpy's one rounding per operation, never a fused multiply-add."""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    factors = [k / 1000 for k in range(3001)] + [1 / 3, 2 / 3, 0.1 + 0.2, np.pi, np.nextafter(1.4, 2.0), -0.5, 1e-300, 255.5]
    descs = [{"op": op, "pixels": ramp, "factor": f, "want": ("pixels",)} for f in factors for op in ("contrast", "brightness")]
    got = []
    for i in range(0, len(descs), 4096):
        got += ctx.image_edit(descs[i:i + 4096])
    for i, f in enumerate(factors):
        assert np.array_equal(got[2 * i]["pixels"], ie.adjust_contrast(ramp, f)), ("contrast", f)
        assert np.array_equal(got[2 * i + 1]["pixels"], ie.adjust_brightness(ramp, f)), ("brightness", f)
    assert int(ie.gpu_edit(ctx, "contrast", ramp[:, 8:9], factor=0.55)[0, 0, 0]) == 62      # (an FMA would give 61)


def test_edits_hash_to_the_reference_hashes(ctx):
    img1, img2 = _data.load_image("img1"), _data.load_image("img2")
    edits = {"img1-grayscale": ie.gpu_edit(ctx, "grayscale", img1), "img1-sharpness": ie.gpu_edit(ctx, "sharpness", img1),
             "img1-blur": ie.gpu_edit(ctx, "blur", img1), "img2-contrast": ie.gpu_edit(None, "contrast", img2, factor=1.4)}
    chain1 = ie.gpu_edit_chain(ctx, img1, [("sharpness", {}), ("grayscale", {})])
    chain2 = ie.gpu_edit_chain(ctx, img2, [("contrast", {"factor": 1.4}), ("sharpness", {})])
    edits["img1-sharpness-grayscale"] = chain1[1][0]
    edits["img2-contrast-sharpness"] = chain2[1][0]
    names = sorted(edits)
    assert image_hasher.image_hashes(ctx, [edits[k] for k in names]) == [int(KAT["hashes"][k]) for k in names]
    assert np.array_equal(chain1[0][0], edits["img1-sharpness"]) and np.array_equal(chain2[0][0], edits["img2-contrast"])
    _assert_input_equal(chain1[1][1], ie.build_input("grayscale", edits["img1-sharpness"]), "chain1")
    _assert_input_equal(chain2[0][1], ie.build_input("contrast", img2, factor=1.4), "chain2")
    _assert_input_equal(chain2[1][1], ie.build_input("sharpness", edits["img2-contrast"]), "chain2")


@pytest.mark.parametrize("op", list(OPS))
def test_inputs_match_pyvimz_rows(ctx, op):
    """gpu_build_input reproduces the rows minted by importing the reference's pyvimz (the parameters of test_input_tooling_matches_pyvimz_rows)."""
    fx = _data.rows10(op)
    img = _data.load_image(fx["image"])
    kw = {}
    if op in ("contrast", "brightness"):
        kw["factor"] = 1.4
    if op == "crop":
        kw.update(x=200, y=100, crop_size="SD")
    if op == "resize":
        kw["resize_to"] = (640, 480)
    inp = ie.gpu_build_input(ctx, op, img, **kw)
    hexes = lambda rows: [[("0x" + format(int(s, 16), "060x")) for s in r] for r in rows]     # noqa: E731
    assert ie.rows_to_hex(inp["original"][:len(fx["original"])]) == hexes(fx["original"])
    if "transformed" in fx:
        assert ie.rows_to_hex(inp["transformed"][:len(fx["transformed"])]) == hexes(fx["transformed"])
    assert (inp["transformed"] is None) == (op == "hash")
    for k in ("factor", "info"):
        if k in fx:
            assert inp[k] == fx[k]
    if "redact" in fx:
        assert inp["redact"][:len(fx["redact"])] == [int(s, 16) for s in fx["redact"]]


def _fold(ctx, op, inp):
    rows, z0 = folding.prepare_input(op, inp, "HD", demo=True)
    circuit, params = folding.prepare_folding(ctx, op, "HD")
    proof = folding.fold_input(params, rows, z0)
    try:
        folding.verify_folded_proof(proof, params, len(rows), z0)
    except Exception:
        proof.close()
        params.free()
        raise
    return proof, params


def test_folded_contrast_proof_from_gpu_input(ctx):
    img = _data.load_image("img2")
    inp = ie.gpu_build_input(ctx, "contrast", img, factor=1.4)
    edited = ie.gpu_edit(ctx, "contrast", img, factor=1.4)
    proof, params = _fold(ctx, "contrast", inp)
    try:
        folding.verify_final_state(proof, "contrast", img, edited, demo=True)
        bad = edited.copy()
        bad[3, 40, 0] ^= 4
        with pytest.raises(_lib.VimzError) as e:
            folding.verify_final_state(proof, "contrast", img, bad, demo=True)
        assert e.value.code == _lib.ERR_UNSAT
    finally:
        proof.close()
        params.free()


def test_folded_redact_proof_with_caller_flags(ctx):
    img = _data.load_image("img1")
    flags = np.zeros((720 // 40) * (1280 // 40), dtype=np.uint8)
    flags[[1, 2, 5, 6, 7, 100, 300]] = 1                         # not pyvimz's checkerboard
    inp = ie.gpu_build_input(ctx, "redact", img, redact=flags)
    assert inp["redact"] == [int(v) for v in flags]
    edited = ie.gpu_edit(ctx, "redact", img, redact=flags)
    want = img.copy()
    for b in np.flatnonzero(flags):
        by, bx = divmod(int(b), 32)
        want[40 * by:40 * by + 40, 40 * bx:40 * bx + 40] = 0
    assert np.array_equal(edited, want)
    assert np.array_equal(inp["transformed"], ie.compress_by_blocks(want)) and np.array_equal(inp["original"], ie.compress_by_blocks(img))
    proof, params = _fold(ctx, "redact", inp)
    try:
        folding.verify_final_state(proof, "redact", img, edited, demo=True, redact=flags)
        bad = edited.copy()
        bad[5, 125, 1] ^= 0x10          # block 3 is not redacted
        with pytest.raises(_lib.VimzError) as e:
            folding.verify_final_state(proof, "redact", img, bad, demo=True, redact=flags)
        assert e.value.code == _lib.ERR_UNSAT
    finally:
        proof.close()
        params.free()


def test_bad_descriptors_are_refused_and_the_context_stays_usable(ctx):
    px = np.zeros((80, 120, 3), dtype=np.uint8)
    grey = np.zeros((80, 120), dtype=np.uint8)
    bad = [
        [{"op": 9, "pixels": px}],                                                               # unknown op
        [{"op": -1, "pixels": px}],
        [{"op": "crop", "pixels": px, "x": 100, "y": 0, "new_width": 40, "new_height": 10}],     # window past the right edge
        [{"op": "crop", "pixels": px, "x": 0, "y": 50, "new_width": 40, "new_height": 40}],      # ... past the bottom
        [{"op": "resize", "pixels": px, "new_width": 120, "new_height": 40}],                    # xl + 1 outside
        [{"op": "resize", "pixels": px, "new_width": 60, "new_height": 80}],                     # yl + 1 outside
        [{"op": "redact", "pixels": px, "redact": [1, 0, 1]}],                                   # 6 blocks
        [{"op": "redact", "pixels": px, "redact": []}],                                          # zero flags: refused, never the checkerboard
        [{"op": "redact", "pixels": px, "redact": [1] * 7}],
        [{"op": "grayscale", "source": 0}],                                                      # not an earlier edit
        [{"op": "grayscale", "pixels": px}, {"op": "blur", "source": 1}],
        [{"op": "grayscale", "pixels": px}, {"op": "contrast", "source": -1, "factor": 1.0}],
        [{"op": "contrast", "pixels": grey, "factor": 1.0}],                                     # grey source for an RGB op
        [{"op": "grayscale", "pixels": px}, {"op": "sharpness", "source": 0}],
        [{"op": "contrast", "pixels": px, "factor": float("inf")}],
        [{"op": "redact", "pixels": np.zeros((41, 37, 3), dtype=np.uint8)}],                     # blocks of a 41 x 37 image
        [],
    ]
    for descs in bad:
        with pytest.raises(_lib.VimzError) as e:
            ctx.image_edit(descs)
        assert e.value.code == _lib.ERR_INVALID, descs
    # more than 2^30 pixels: refused from the sizes alone, before the (here tiny) buffer is read
    tiny = np.zeros(16, dtype=np.uint8)
    arr = (hip.EditDesc * 1)()
    arr[0].op, arr[0].pixels, arr[0].height, arr[0].width, arr[0].channels = 0, tiny.ctypes.data, 1 << 16, (1 << 14) + 1, 3
    shapes = (hip.EditShape * 1)()
    ctx.lib.vimz_image_edit_shapes.argtypes = [hip.C.c_void_p, hip.C.POINTER(hip.EditDesc), hip.C.c_size_t, hip.C.POINTER(hip.EditShape)]
    ctx.lib.vimz_image_edit.argtypes = [hip.C.c_void_p, hip.C.POINTER(hip.EditDesc), hip.C.c_size_t]
    assert ctx.lib.vimz_image_edit_shapes(ctx.h, arr, 1, shapes) == _lib.ERR_INVALID
    assert ctx.lib.vimz_image_edit(ctx.h, arr, 1) == _lib.ERR_INVALID
    img = _data.load_image("img2")[:50]
    assert np.array_equal(ie.gpu_edit(ctx, "contrast", img, factor=0.7), ie.adjust_contrast(img, 0.7))
    _assert_input_equal(ie.gpu_build_input(ctx, "blur", img), ie.build_input("blur", img), "after refusals")


def test_last_profile_splits_the_call(ctx):
    img = _upscaled(3)
    for _ in range(2):
        ie.gpu_build_input(ctx, "sharpness", img)
    p = ctx.image_edit_last_profile()
    assert set(p) == {"upload", "kernels", "download"} and all(v > 0 for v in p.values())


def test_command_line_writes_the_input_and_the_png(ctx, tmp_path, golden_dir):
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    flags = tmp_path / "flags.json"
    flags.write_text(json.dumps([0, 1] + [0] * 574))
    img1, img2 = _data.load_image("img1"), _data.load_image("img2")
    runs = [(["contrast", "-i", os.path.join(golden_dir, "img2.png"), "--factor", "1.4"], ie.build_input("contrast", img2, factor=1.4),
             ie.adjust_contrast(img2, 1.4)),
            (["resize", "-i", os.path.join(golden_dir, "img1.png"), "--resize-option", "HD to SD"], ie.build_input("resize", img1, resize_to=(640, 480)),
             ie.resize_image(img1, 480, 640))]
    red = img1.copy()
    red[0:40, 40:80] = 0
    runs.append((["redact", "-i", os.path.join(golden_dir, "img1.png"), "--redact-flags", str(flags)], None, red))
    for args, inp, png in runs:
        out, pic = tmp_path / f"{args[0]}.json", tmp_path / f"{args[0]}.png"
        r = subprocess.run([sys.executable, "-m", "vimz_amd.image_editor", *args, "-o", str(out), "--save-png", str(pic)], cwd=root, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        if inp is not None:
            ie.dump_json(inp, tmp_path / "want.json")
            assert out.read_text() == (tmp_path / "want.json").read_text(), args[0]
        else:
            got = ie.load_json(out)
            assert got["redact"] == [0, 1] + [0] * 574
            assert np.array_equal(got["transformed"], ie.compress_by_blocks(red))
        assert np.array_equal(np.array(Image.open(pic)), png), args[0]
    # an empty flags file is zero flags, not "no flags": refused, and nothing is written
    empty = tmp_path / "empty.txt"
    empty.write_text("")
    out, pic = tmp_path / "empty.json", tmp_path / "empty.png"
    r = subprocess.run([sys.executable, "-m", "vimz_amd.image_editor", "redact", "-i", os.path.join(golden_dir, "img1.png"), "--redact-flags",
                        str(empty), "-o", str(out), "--save-png", str(pic)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "one flag per full 40 x 40 block" in r.stderr, r.stderr
    assert not out.exists() and not pic.exists()
