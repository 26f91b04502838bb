"""vimz_image_hash on the MI355X: the reference's image hashes, agreement with the CPU oracle on every Poseidon width the digests use, and a
folded proof's final state checked against its images (vimz_amd.folding.verify_final_state)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _data
from tests import _image_hash_oracle as iho
from vimz_amd import _lib, folding, hip, image_hasher
from vimz_amd import image_editor as ie

pytestmark = pytest.mark.gpu

KAT = _data.kat()
NAMES = sorted(KAT["hashes"])


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def images():
    img1, img2 = _data.load_image("img1"), _data.load_image("img2")
    sharp, con = ie.sharpen_image(img1), ie.adjust_contrast(img2, 1.4)
    return {"img1": img1, "img2": img2, "img1-grayscale": ie.convert_to_grayscale(img1), "img2-contrast": con, "img1-sharpness": sharp,
            "img1-blur": ie.blur_image(img1), "img1-sharpness-grayscale": ie.convert_to_grayscale(sharp),
            "img2-contrast-sharpness": ie.sharpen_image(con)}


def test_reference_hashes_one_per_call(ctx, images):
    for k in NAMES:
        assert image_hasher.image_hash(ctx, images[k]) == int(KAT["hashes"][k]), k


def test_reference_hashes_in_one_call(ctx, images):
    assert image_hasher.image_hashes(ctx, [images[k] for k in NAMES]) == [int(KAT["hashes"][k]) for k in NAMES]


LENGTHS = [1, 7, 8, 9, 15, 16, 64, 128, 160, 192, 768]     # every width t = 2..9, window edges at 8, 9, 15, 16


def _random_units(rng, n, L):
    b = np.zeros((n, L, 32), dtype=np.uint8)
    b[:, :, :30] = rng.integers(0, 256, size=(n, L, 30), dtype=np.uint8)     # 240-bit elements, as packed pixels are
    return b.view("<u8").reshape(n, L, 4)


def test_packed_units_match_oracle_every_length(ctx, oracle):
    rng = np.random.default_rng(1)
    units = [_random_units(rng, 3, L) for L in LENGTHS]
    got = image_hasher.image_hashes(ctx, units)                 # (all lengths in one launch)
    for L, u, g in zip(LENGTHS, units, got):
        assert g == iho.image_hash(oracle, {"image": u}), L
    assert [image_hasher.image_hash(ctx, u) for u in units[:4]] == got[:4]


def test_pixel_rows_match_oracle_every_length(ctx, oracle):
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, size=(3, max(1, 10 * L - 3), 3), dtype=np.uint8) for L in LENGTHS]     # (last element of a row partly padding)
    got = image_hasher.image_hashes(ctx, imgs)
    for L, img, g in zip(LENGTHS, imgs, got):
        assert g == iho.image_hash(oracle, {"image": img}), L


def test_grey_rgba_and_max_units(ctx, oracle):
    rng = np.random.default_rng(3)
    grey = rng.integers(0, 256, size=(6, 95), dtype=np.uint8)
    rgba = rng.integers(0, 256, size=(6, 95, 4), dtype=np.uint8)
    g = image_hasher.image_hashes(ctx, [grey, rgba, {"image": rgba, "units": 4}, grey[:, :, None]])
    assert g[0] == iho.image_hash(oracle, {"image": grey}) == g[3]
    assert g[1] == iho.image_hash(oracle, {"image": rgba[:, :, :3]})
    assert g[2] == iho.image_hash(oracle, {"image": rgba, "units": 4}) != g[1]


def test_blocks_with_and_without_drop(ctx, oracle):
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(80, 120, 3), dtype=np.uint8)     # 2 x 3 blocks of 40 x 40
    drop = [0, 1, 0, 0, 1, 1]
    specs = [{"image": img, "mode": "blocks"}, {"image": img, "mode": "blocks", "drop": drop}, {"image": img, "mode": "blocks", "units": 4, "drop": drop[:4]},
             {"image": img, "mode": "blocks", "drop": [1] * 6}]
    got = image_hasher.image_hashes(ctx, specs)
    assert got == [iho.image_hash(oracle, s) for s in specs]
    assert len(set(got)) == 4


@pytest.mark.parametrize("resolution,rows", [("4K", 6), ("8K", 3)])
def test_4k_8k_rows_match_oracle(ctx, oracle, resolution, rows):
    k = {"4K": 3, "8K": 6}[resolution]
    src = _data.load_image("img2")[: (rows + k - 1) // k + 1]
    img = np.repeat(np.repeat(src, k, axis=0), k, axis=1)[:rows]       # (as tests/_data.config_rows upscales img2)
    assert img.shape[1] == {"4K": 3840, "8K": 7680}[resolution]
    assert image_hasher.image_hash(ctx, img) == iho.image_hash(oracle, {"image": img})


def _fold_and_check(ctx, transformation, img, **kw):
    inp = ie.build_input(transformation, img, **kw)
    rows, z0 = folding.prepare_input(transformation, inp, "HD", demo=True)
    circuit, params = folding.prepare_folding(ctx, transformation, "HD")
    proof = folding.fold_input(params, rows, z0)
    try:
        folding.verify_folded_proof(proof, params, len(rows), z0)
        return proof, params, inp
    except Exception:
        proof.close()
        params.free()
        raise


def test_folded_hash_proof_against_its_image(ctx, images):
    proof, params, _ = _fold_and_check(ctx, "hash", images["img2"])
    try:
        folding.verify_final_state(proof, "hash", images["img2"], demo=True)
        with pytest.raises(_lib.VimzError, match="Source image hash does not match final state"):
            folding.verify_final_state(proof, "hash", images["img1"], demo=True)
    finally:
        proof.close()
        params.free()


def test_folded_contrast_proof_against_its_images(ctx, images):
    proof, params, _ = _fold_and_check(ctx, "contrast", images["img2"], factor=1.4)
    try:
        folding.verify_final_state(proof, "contrast", images["img2"], images["img2-contrast"], demo=True)
        folding.verify_final_state(proof.state(), "contrast", images["img2"], images["img2-contrast"], demo=True, hasher=ctx)
        bad = images["img2-contrast"].copy()
        bad[3, 40, 0] ^= 4
        with pytest.raises(_lib.VimzError, match="Target image hash does not match final state"):
            folding.verify_final_state(proof, "contrast", images["img2"], bad, demo=True)
        with pytest.raises(_lib.VimzError, match="Source image hash"):
            folding.verify_final_state(proof, "contrast", images["img2-contrast"], images["img2"], demo=True)
        with pytest.raises(_lib.VimzError):
            folding.verify_final_state(proof, "contrast", images["img2"], images["img2-contrast"])       # (10 steps, not 720)
    finally:
        proof.close()
        params.free()


def test_folded_redact_proof_against_its_images(ctx, images):
    proof, params, inp = _fold_and_check(ctx, "redact", images["img1"])
    red, flags = ie.random_image_redaction(images["img1"])
    assert flags == inp["redact"]
    try:
        folding.verify_final_state(proof, "redact", images["img1"], red, demo=True, redact=flags)
        bad = red.copy()
        bad[5, 5, 0] ^= 0x40      # block 0 is not redacted: a pixel of it changed changes the target
        with pytest.raises(_lib.VimzError, match="Target image hash does not match final state"):
            folding.verify_final_state(proof, "redact", images["img1"], bad, demo=True, redact=flags)
        with pytest.raises(_lib.VimzError) as e:
            folding.verify_final_state(proof, "redact", images["img1"], red, demo=True)
        assert e.value.code == _lib.ERR_INVALID
    finally:
        proof.close()
        params.free()


def test_command_line_writes_the_hash_file(tmp_path, golden_dir):
    out = tmp_path / "img2.hash"
    env = dict(os.environ)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "vimz_amd.image_hasher", os.path.join(golden_dir, "img2.png"), str(out)], cwd=root, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == KAT["hashes"]["img2"]
    assert out.read_bytes() == KAT["hashes"]["img2"].encode()


def test_bad_descriptors_are_refused_and_the_context_stays_usable(ctx):
    px = np.zeros((4, 20, 3), dtype=np.uint8)
    P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    big = np.zeros((1, 2, 4), dtype=np.uint64)
    for k in range(4):
        big[0, 1, k] = (P >> (64 * k)) & 0xFFFFFFFFFFFFFFFF       # an element equal to the modulus
    bad = [
        [{"pixels": np.zeros((4, 20, 2), dtype=np.uint8)}],       # two channels
        [{"pixels": px, "block": 5000}],
        [{"pixels": px, "block": -1}],
        [{"pixels": px, "max_units": 5}],                          # more rows than the image has
        [{"pixels": px, "max_units": 2}, {"pixels": px, "block": 40, "max_units": 2}],
        [{"units": big}],
        [{"units": np.zeros((2, 3, 4), dtype=np.uint64), "block": 40}],
        [],
    ]
    for descs in bad:
        with pytest.raises(_lib.VimzError) as e:
            ctx.image_hash(descs)
        assert e.value.code == _lib.ERR_INVALID, descs
    ok = ctx.image_hash([{"pixels": px}, {"units": big[:, :1]}])
    assert ok == image_hasher.image_hashes(ctx, [px, big[:, :1]])
    assert ok[0] != 0
