"""The GPU image editor's command line and Python layer without a GPU: usage errors are reported before any device is opened, and there is no
CPU fallback."""
import os
import subprocess
import sys

import numpy as np
import pytest

from vimz_amd import _lib
from vimz_amd import image_editor as ie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = os.path.join(ROOT, "tests", "golden", "img2.png")


def _cli(*args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "vimz_amd.image_editor", *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("args,message", [
    ((), "required"),                                                               # no operation, no image
    (("contrast",), "--image-path"),                                                # no image
    (("sepia", "-i", IMG), "invalid choice"),                                       # unknown operation
    (("contrast", "-i", IMG), "needs --factor"),
    (("brightness", "-i", IMG), "needs --factor"),
    (("crop", "-i", IMG, "--x", "10", "--y", "10"), "needs --x, --y and --crop-size"),
    (("crop", "-i", IMG, "--x", "10", "--crop-size", "SD"), "needs --x, --y and --crop-size"),
    (("crop", "-i", IMG, "--x", "1", "--y", "1", "--crop-size", "XL"), "invalid choice"),
    (("resize", "-i", IMG), "needs --resize-option"),
    (("resize", "-i", IMG, "--resize-option", "HD to FHD"), "invalid choice"),
    (("grayscale", "-i", IMG, "--redact-flags", "flags.json"), "for redact only"),
    (("contrast", "-i", IMG, "--factor", "high"), "invalid float"),
])
def test_command_line_usage_errors(args, message):
    r = _cli(*args)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr


def test_command_line_unreadable_inputs(tmp_path):
    r = _cli("grayscale", "-i", str(tmp_path / "missing.png"), "-o", str(tmp_path / "out.json"))
    assert r.returncode == 1 and "image_editor:" in r.stderr
    bad = tmp_path / "flags.txt"
    bad.write_text('{"not": "a list"}')
    r = _cli("redact", "-i", IMG, "--redact-flags", str(bad), "-o", str(tmp_path / "out.json"))
    assert r.returncode == 1 and "not a list of flags" in r.stderr
    assert not (tmp_path / "out.json").exists()


def test_redact_flag_files(tmp_path):
    for text, want in (("[0, 1, 1]", [0, 1, 1]), ('["0x0", "0x1"]', [0, 1]), ("1 0\n1\n", [1, 0, 1]), ('{"redact": ["0x1"]}', [1])):
        p = tmp_path / "f"
        p.write_text(text)
        assert ie._read_flags(str(p)) == want


def test_parameters_are_checked_before_the_device():
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for op, kw in (("sepia", {}), ("contrast", {}), ("crop", {"x": 1, "y": 1}), ("crop", {"x": 1, "y": 1, "crop_size": "XL"}), ("resize", {})):
        with pytest.raises(ValueError):
            ie.gpu_edit(None, op, img, **kw)
    with pytest.raises(ValueError):
        ie.gpu_build_input(None, "grayscale", img.astype(np.float32))


def test_input_fields_follow_build_input():
    assert ie._input_fields("contrast", {"factor": 1.4}, (720, 1280, 3)) == {"factor": 14}
    assert ie._input_fields("crop", {"x": 200, "y": 100}, (720, 1280, 3)) == {"info": 200 * 2 ** 24 + 100 * 2 ** 12}
    img = np.zeros((120, 200, 3), dtype=np.uint8)
    assert ie._input_fields("redact", {"redact": None}, img.shape) == {"redact": ie.random_image_redaction(img)[1]}
    assert ie._input_fields("redact", {"redact": np.array([0, 3, 1])}, img.shape) == {"redact": [0, 1, 1]}


def test_no_cpu_fallback_without_gpu():
    """Without a GPU the editor fails loudly instead of editing with numpy."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    img = np.zeros((16, 16, 3), dtype=np.uint8)
    for call in (lambda: ie.gpu_build_input(None, "contrast", img, factor=1.4), lambda: ie.gpu_edit(None, "grayscale", img),
                 lambda: ie.gpu_edit_chain(None, img, [("sharpness", {}), ("grayscale", {})])):
        with pytest.raises(_lib.VimzError) as e:
            call()
        assert e.value.code == _lib.ERR_NO_DEVICE
    r = _cli("contrast", "-i", IMG, "--factor", "1.4", "-o", os.devnull)
    assert r.returncode == 1 and "image_editor:" in r.stderr


# ---- the kernels' thread code on the CPU (tests/native/image_edit_host.hip, built by `make all`), driven through hip.Context.image_edit

class _HostEditLib:
    """Stands in for the product library under hip.Context.image_edit: the two calls go to the host build of image_edit.hip."""

    class _Fn:
        def __init__(self, f):
            self.f, self.argtypes = f, None

        def __call__(self, *a):
            return self.f(*a)

    def __init__(self, so):
        import ctypes as C
        so.edit_host_last_error.restype = C.c_char_p
        self._so = so
        self.vimz_image_edit_shapes = self._Fn(lambda h, arr, n, out: so.edit_host_shapes(arr, C.c_size_t(n), out))
        self.vimz_image_edit = self._Fn(lambda h, arr, n: so.edit_host_run(arr, C.c_size_t(n)))

    def vimz_last_error(self, h):
        return self._so.edit_host_last_error()


@pytest.fixture(scope="module")
def host_ctx():
    import ctypes
    from vimz_amd import hip
    path = os.path.join(ROOT, "vimz_amd", "csrc", "build", "libimage_edit_host.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    c = object.__new__(hip.Context)
    c.lib, c.h, c.device = _HostEditLib(ctypes.CDLL(path)), None, -1
    return c


def _host_params(op, img):
    h, w = img.shape[:2]
    if op in ("contrast", "brightness"):
        return {"factor": 1.4}
    if op == "crop":
        return {"x": 200, "y": 100, "crop_size": "SD"} if h >= 580 and w >= 840 else {"x": w // 3, "y": h // 3, "crop_size": (w // 2, h // 2)}
    if op == "resize":
        return {"resize_to": (640, 480)} if h == 720 else {"resize_to": (w // 2, h // 2)}
    return {}


def _host_reference(op, img, p):
    img = img[..., :3]
    fns = {"grayscale": ie.convert_to_grayscale, "blur": ie.blur_image, "sharpness": ie.sharpen_image, "hash": lambda a: a,
           "redact": lambda a: ie.random_image_redaction(a)[0], "contrast": lambda a: ie.adjust_contrast(a, p["factor"]),
           "brightness": lambda a: ie.adjust_brightness(a, p["factor"])}
    if op == "crop":
        w, h = ie._crop_wh(p["crop_size"])
        return ie.crop_image(img, p["x"], p["y"], w, h)
    if op == "resize":
        w, h = p["resize_to"]
        return ie.resize_image(img, h, w)
    return fns[op](img)


@pytest.mark.parametrize("shape", [(720, 1280, 3), (120, 200, 3), (41, 37, 3), (80, 95, 4)])
def test_thread_code_matches_the_host_editor(host_ctx, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    blocks = shape[0] % 40 == 0 and shape[1] % 40 == 0
    for op in ie.OPERATIONS:
        p = _host_params(op, img)
        assert np.array_equal(ie.gpu_edit(host_ctx, op, img, **p), _host_reference(op, img, p)), (shape, op)
        if op == "redact" and not blocks:
            with pytest.raises(_lib.VimzError) as e:
                ie.gpu_build_input(host_ctx, op, img, **p)
            assert e.value.code == _lib.ERR_INVALID
            continue
        got = ie.gpu_build_input(host_ctx, op, img, **p)
        if isinstance(p.get("crop_size", ""), str):
            want = ie.build_input(op, img, **p)
            assert np.array_equal(got["original"], want["original"]), (shape, op)
            assert (want["transformed"] is None and got["transformed"] is None) or np.array_equal(got["transformed"], want["transformed"]), (shape, op)
            assert {k: got.get(k) for k in ("factor", "info", "redact")} == {k: want.get(k) for k in ("factor", "info", "redact")}


def test_thread_code_chains_flags_and_rounding(host_ctx):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, size=(80, 120, 3), dtype=np.uint8)
    (s, _), (g, inp) = ie.gpu_edit_chain(host_ctx, img, [("sharpness", {}), ("grayscale", {})])
    assert np.array_equal(s, ie.sharpen_image(img)) and np.array_equal(g, ie.convert_to_grayscale(ie.sharpen_image(img)))
    assert np.array_equal(inp["original"], ie.compress_by_rows(s)) and np.array_equal(inp["transformed"], ie.compress_by_rows(g))
    flags = [0, 0, 1, 1, 0, 1]
    red = img.copy()
    red[0:40, 80:120] = 0
    red[40:80, 0:40] = 0
    red[40:80, 80:120] = 0
    inp = ie.gpu_build_input(host_ctx, "redact", img, redact=flags)
    assert inp["redact"] == flags and np.array_equal(inp["transformed"], ie.compress_by_blocks(red))
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    factors = [k / 1000 for k in range(3001)] + [1 / 3, 0.1 + 0.2]
    descs = [{"op": "contrast", "pixels": ramp, "factor": f, "want": ("pixels",)} for f in factors]
    got = host_ctx.image_edit(descs[:4096])
    for f, r in zip(factors, got):
        assert np.array_equal(r["pixels"], ie.adjust_contrast(ramp, f)), f


def test_thread_code_refusals(host_ctx):
    px = np.zeros((80, 120, 3), dtype=np.uint8)
    bad = [
        [{"op": "redact", "pixels": px, "redact": []}],            # zero flags are not "no flags": refused, never the checkerboard
        [{"op": "redact", "pixels": px, "redact": [1, 0, 1]}],
        [{"op": "crop", "pixels": px, "x": 100, "y": 0, "new_width": 40, "new_height": 10}],
        [{"op": "resize", "pixels": px, "new_width": 120, "new_height": 40}],
        [{"op": "grayscale", "pixels": px}, {"op": "blur", "source": 0}],
        [{"op": "grayscale", "source": 0}],
        [{"op": 9, "pixels": px}],
    ]
    for descs in bad:
        with pytest.raises(_lib.VimzError) as e:
            host_ctx.image_edit(descs)
        assert e.value.code == _lib.ERR_INVALID, descs
    with pytest.raises(_lib.VimzError, match="one flag per full 40 x 40 block"):
        ie.gpu_edit(host_ctx, "redact", px, redact=[])
    # an image without a full block takes an empty flag list
    small = np.full((30, 30, 3), 7, dtype=np.uint8)
    assert np.array_equal(ie.gpu_edit(host_ctx, "redact", small, redact=[]), small)
