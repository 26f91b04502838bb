"""A proof's final state against its images (vimz_amd.folding.expected_final_state / verify_final_state) with the CPU oracle as the hasher:
the rules per transformation reproduce the final states of the reference's committed proofs, and refuse what they must.  No GPU needed."""
import numpy as np
import pytest

from tests import _data
from tests import _image_hash_oracle as iho
from tests._oracle import T_CROP, T_REDACT, T_RESIZE, from_limbs
from vimz_amd import _lib, folding, image_hasher
from vimz_amd import image_editor as ie

KAT = _data.kat()


@pytest.fixture(scope="module")
def images():
    img1, img2 = _data.load_image("img1"), _data.load_image("img2")
    sharp, con = ie.sharpen_image(img1), ie.adjust_contrast(img2, 1.4)
    return {"img1": img1, "img2": img2, "img1-grayscale": ie.convert_to_grayscale(img1), "img2-contrast": con, "img1-sharpness": sharp,
            "img1-blur": ie.blur_image(img1), "img1-sharpness-grayscale": ie.convert_to_grayscale(sharp),
            "img2-contrast-sharpness": ie.sharpen_image(con)}


@pytest.fixture(scope="module")
def hasher(oracle):
    return iho.hasher(oracle)


# (proof, transformation, source image, target image) of the six proofs the reference commits (marketplace/proofs)
PROOFS = [
    ("img1-blur", "blur", "img1", "img1-blur"),
    ("img1-grayscale", "grayscale", "img1", "img1-grayscale"),
    ("img1-sharpness", "sharpness", "img1", "img1-sharpness"),
    ("img1-sharpness-grayscale", "grayscale", "img1-sharpness", "img1-sharpness-grayscale"),
    ("img2-contrast", "contrast", "img2", "img2-contrast"),
    ("img2-contrast-sharpness", "sharpness", "img2-contrast", "img2-contrast-sharpness"),
]


@pytest.mark.parametrize("proof,transformation,src,tgt", PROOFS)
def test_expected_final_state_reproduces_committed_proofs(images, hasher, proof, transformation, src, tgt):
    z = [int(v) for v in KAT["proofs"][proof]["z_final"]]
    exp = folding.expected_final_state(transformation, images[src], images[tgt], hasher=hasher)
    assert exp == {0: z[0], 1: z[1]}
    assert exp[0] == int(KAT["hashes"][src]) and exp[1] == int(KAT["hashes"][tgt])
    folding.verify_final_state(z, transformation, images[src], images[tgt], hasher=hasher)


def test_blur_source_is_the_unpadded_image(images, hasher):
    # the blur circuit hashes the middle of its three (zero-padded) rows: z[0] of img1-blur is hash(img1) itself
    z = [int(v) for v in KAT["proofs"]["img1-blur"]["z_final"]]
    assert z[0] == int(KAT["hashes"]["img1"])
    assert folding.expected_final_state("blur", images["img1"], None, hasher=hasher) == {0: z[0]}


def test_swapped_images_are_refused(images, hasher):
    z = [int(v) for v in KAT["proofs"]["img1-grayscale"]["z_final"]]
    with pytest.raises(_lib.VimzError) as e:
        folding.verify_final_state(z, "grayscale", images["img1-grayscale"], images["img1"], hasher=hasher)
    assert e.value.code == _lib.ERR_UNSAT and "Source image hash does not match final state" in str(e.value)


def test_one_changed_pixel_is_refused(images, hasher):
    z = [int(v) for v in KAT["proofs"]["img2-contrast"]["z_final"]]
    src = images["img2"].copy()
    src[400, 17, 1] ^= 1
    with pytest.raises(_lib.VimzError) as e:
        folding.verify_final_state(z, "contrast", src, images["img2-contrast"], hasher=hasher)
    assert e.value.code == _lib.ERR_UNSAT and "Source image" in str(e.value)
    tgt = images["img2-contrast"].copy()
    tgt[719, 500, 2] ^= 0x80      # (not past pixel 1129 of a row: ArrayHasher(128) absorbs 113 of its 128 elements)
    with pytest.raises(_lib.VimzError) as e:
        folding.verify_final_state(z, "contrast", images["img2"], tgt, hasher=hasher)
    assert e.value.code == _lib.ERR_UNSAT and "Target image hash does not match final state" in str(e.value)
    folding.verify_final_state(z, "contrast", images["img2"], None, hasher=hasher)      # (what is not given is not checked)


def _oracle_chain(oracle, t, rows, z0, **shape):
    z = list(z0)
    for r in rows:
        ok, z = oracle.step_eval(t, z, r, **shape)
        assert ok
    return z


def test_redact_demo(oracle, images, hasher):
    img = images["img1"]
    inp = ie.build_input("redact", img)
    rows, z0 = folding.prepare_input("redact", inp, "HD", demo=True)
    z = _oracle_chain(oracle, T_REDACT, rows, z0, width=160)
    red, flags = ie.random_image_redaction(img)
    assert any(flags[:folding.DEMO_STEPS])
    assert folding.expected_final_state("redact", img, red, demo=True, redact=flags, hasher=hasher) == {0: z[0], 1: z[1]}
    folding.verify_final_state(z, "redact", img, red, demo=True, redact=flags, hasher=hasher)
    # a redacted block enters as PairHasher(acc, 0), not as the digest of a black block: without the flags the target cannot be checked
    with pytest.raises(_lib.VimzError) as e:
        folding.expected_final_state("redact", img, red, demo=True, hasher=hasher)
    assert e.value.code == _lib.ERR_INVALID
    black = hasher([{"image": red, "mode": "blocks", "units": folding.DEMO_STEPS}])[0]
    assert black != z[1]
    assert folding.expected_final_state("redact", img, None, demo=True, hasher=hasher) == {0: z[0]}
    # a flag set where the target's block was not redacted is a different statement
    wrong = list(flags)
    wrong[0] = 1
    with pytest.raises(_lib.VimzError, match="Target image hash"):
        folding.verify_final_state(z, "redact", img, red, demo=True, redact=wrong, hasher=hasher)


def test_resize_demo_hashes_3n_source_and_2n_target_rows(oracle, images, oracle_hasher_fresh):
    img = images["img1"]
    inp = ie.build_input("resize", img, resize_to=(640, 480))
    rows, z0 = folding.prepare_input("resize", inp, "HD", demo=True)
    z = _oracle_chain(oracle, T_RESIZE, rows, z0, width=128, width2=64, rows_in=3, rows_out=2)
    small = ie.resize_image(img, 480, 640)
    h = oracle_hasher_fresh
    assert folding.expected_final_state("resize", img, small, demo=True, hasher=h) == {0: z[0], 1: z[1]}
    (specs,) = h.calls
    assert [s["units"] for s in specs] == [3 * folding.DEMO_STEPS, 2 * folding.DEMO_STEPS]
    assert folding.final_state_units("resize", "HD") == (240, 720, 480)


@pytest.fixture
def oracle_hasher_fresh(oracle):
    return iho.hasher(oracle)


def test_crop_target_is_not_the_hash_of_the_cropped_image(oracle, images, hasher):
    """SURVEY.md F6, confirmed on the oracle: the crop circuit's z[1] is NOT the row-wise hash of image_editor.crop_image(...) — the circuit decodes
    x, y and the row index from other bit fields than `info = x·2^24 + y·2^12` sets, and packs only the R byte of each cropped pixel.  So the
    target check is refused (as the reference skips crop's target in demo mode); the source check holds."""
    img = images["img1"]
    x, y = 200, 100
    inp = ie.build_input("crop", img, x=x, y=y, crop_size="SD")
    rows, z0 = folding.prepare_input("crop", inp, "HD", demo=True)
    z = _oracle_chain(oracle, T_CROP, rows, z0, width=128, width2=64, crop_h=480)
    cropped = ie.crop_image(img, x, y, 640, 480)
    as_rows = hasher([{"image": cropped, "units": folding.DEMO_STEPS}])[0]
    assert z[1] != 0 and z[1] != as_rows
    assert folding.expected_final_state("crop", img, None, demo=True, hasher=hasher) == {0: z[0]}
    with pytest.raises(_lib.VimzError) as e:
        folding.verify_final_state(z, "crop", img, cropped, demo=True, hasher=hasher)
    assert e.value.code == _lib.ERR_INVALID and "crop" in str(e.value)


def test_hash_determines_the_source_only(images, hasher, oracle):
    rows, z0 = folding.prepare_input("hash", ie.build_input("hash", images["img2"]), "HD", demo=True)
    z = list(z0)
    for r in rows:
        z = [oracle.head_tail_hash(z[0], from_limbs(r))]
    folding.verify_final_state(z, "hash", images["img2"], demo=True, hasher=hasher)
    with pytest.raises(_lib.VimzError) as e:
        folding.verify_final_state(z, "hash", images["img2"], images["img2"], demo=True, hasher=hasher)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.VimzError, match="Source image"):
        folding.verify_final_state(z, "hash", images["img1"], demo=True, hasher=hasher)


def test_request_validation():
    img = np.zeros((30, 25, 3), dtype=np.uint8)
    assert image_hasher._desc({"image": img})["max_units"] == 30
    assert image_hasher._desc({"image": img, "mode": "blocks"})["max_units"] == 1
    for bad in ({"units": 31}, {"units": 0}, {"drop": [0] * 29}, {"mode": "cols"}):
        with pytest.raises(ValueError):
            image_hasher._desc(dict({"image": img}, **bad))
    for arr in (np.zeros((4, 4, 2), np.uint8), np.zeros((4, 4, 3), np.uint16), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            image_hasher._desc({"image": arr})
    d = image_hasher._desc({"image": img[:, :, :1], "drop": [1, 0, 2] + [0] * 27})
    assert d["pixels"].ndim == 2 and list(d["drop"][:3]) == [1, 0, 1]
    with pytest.raises(ValueError):
        image_hasher._desc({"image": np.zeros((3, 4, 4), np.uint64), "mode": "blocks"})
