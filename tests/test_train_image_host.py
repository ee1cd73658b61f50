"""CPU: the host side of the training image preparation (chore_amd/data/train_image_prep.py) and the numpy reference the
GPU tests use (tests/train_image_ref.py), pinned against PIL itself and against the fixture that the reference's
BaseDataset.blur_image wrote (tests/golden/make_train_image_golden.py)."""
import os

import numpy as np
import pytest

from train_image_ref import box_params_ref, pil_blur_ref

RADII = (0, 0.3, 0.9, 1.7, 2.55, 6.2, 12.75, 40)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "train_image_prep.npz"))


def _images():
    rs = np.random.RandomState(3)
    return rs.randint(0, 256, (37, 53)).astype(np.uint8), rs.randint(0, 256, (64, 48, 3)).astype(np.uint8)


@pytest.mark.parametrize("radius", RADII)
def test_restatement_equals_pil(radius):
    Image = pytest.importorskip("PIL.Image")
    from PIL.ImageFilter import GaussianBlur
    for img in _images():
        want = np.array(Image.fromarray(img).filter(GaussianBlur(radius)))
        assert np.array_equal(pil_blur_ref(img, radius), want), (radius, img.shape)


def test_restatement_equals_pil_where_double_arithmetic_does_not():
    """PIL computes the effective box radius in float32; in double this radius gives a weight one unit off and an image one
    grey level off"""
    Image = pytest.importorskip("PIL.Image")
    from PIL.ImageFilter import GaussianBlur
    r = 0.7881700701273976
    assert box_params_ref(r)[1:] == (0, 13303146, 1737035)        # all in double: (0, 13303147, 1737034)
    for img in _images():
        assert np.array_equal(pil_blur_ref(img, r), np.array(Image.fromarray(img).filter(GaussianBlur(r))))


def test_restatement_equals_the_reference_fixture(golden):
    for want, radius in zip(golden["blurred"], golden["radius"]):
        assert np.array_equal(pil_blur_ref(golden["image"], radius), want), radius
    assert not np.array_equal(golden["blurred"][2], golden["image"])


@pytest.mark.parametrize("radius", (0.9, 12.75))
def test_mirror_and_blur_commute(radius):
    """what lets the compose kernel mirror by index AFTER the blur: in the restatement and in PIL"""
    _, img = _images()
    mirrored = np.ascontiguousarray(img[:, ::-1])
    assert np.array_equal(pil_blur_ref(mirrored, radius), pil_blur_ref(img, radius)[:, ::-1])
    Image = pytest.importorskip("PIL.Image")
    from PIL.ImageFilter import GaussianBlur
    a = np.array(Image.fromarray(mirrored).filter(GaussianBlur(radius)))
    assert np.array_equal(a, np.array(Image.fromarray(img).filter(GaussianBlur(radius)))[:, ::-1])


def test_draws_equal_the_reference_sequence(golden):
    from chore_amd.data import TrainImagePrep
    n = len(golden["draw_flip"])
    prep = TrainImagePrep(random_flip=True, aug_blur=float(golden["draw_aug_blur"]), seed=int(golden["draw_seed"]), device="cpu")
    flips, radii = prep.draw(n)
    assert np.array_equal(flips, golden["draw_flip"]) and np.array_equal(radii, golden["draw_radius"])
    assert flips.any() and not flips.all()
    # the radius alone, as blur_image draws it ('val': get_item draws no flip; 'train' draws one even without random_flip)
    for aug, seed, want in zip(golden["aug_blur"], golden["blur_seed"], golden["radius"]):
        assert TrainImagePrep(phase="val", aug_blur=float(aug), seed=int(seed), device="cpu").draw(1)[1][0] == want
        assert TrainImagePrep(aug_blur=float(aug), seed=int(seed), device="cpu").draw(1)[1][0] != want
    # 'val' draws no flip, and no radius without aug_blur: the stream is untouched
    prep = TrainImagePrep(phase="val", random_flip=True, seed=7, device="cpu")
    flips, radii = prep.draw(3)
    assert not flips.any() and not radii.any() and prep.rng.rand() == np.random.RandomState(7).rand()
    # given values are used as they are and draw nothing
    prep = TrainImagePrep(random_flip=True, aug_blur=0.05, seed=7, device="cpu")
    flips, radii = prep.draw(2, flip=[True, False], blur_radius=[1.5, 0.0])
    assert list(flips) == [True, False] and list(radii) == [1.5, 0.0] and prep.rng.rand() == np.random.RandomState(7).rand()


def test_box_params():
    from chore_amd.data import TrainImagePrep
    assert TrainImagePrep.box_params(0) == (0, 0, 0)
    for r in RADII + (0.7881700701273976, 0.09193754132715229, 9.915705734816207, 63.9):
        R, ww, fw = TrainImagePrep.box_params(r)
        assert (R, ww, fw) == tuple(box_params_ref(r)[1:]), r
        if r:
            assert 0 <= (1 << 24) - ((2 * R + 1) * ww + 2 * fw) <= 1 and fw >= 0      # the weights add to 2^24 (or one less)
    # by hand: r = 2.55 -> sigma^2 = 2.1675, L = sqrt(27.01) = 5.197.., l = 2, a = 5 * (6 - 6.5025) / (6 * (2.1675 - 9)) =
    # 0.061288.., box radius 2.061288..
    R, ww, fw = TrainImagePrep.box_params(2.55)
    assert R == 2 and abs(ww - (1 << 24) / (2 * 2.061288 + 1)) < 40 and TrainImagePrep.box_params(40)[0] == 39
    with pytest.raises(ValueError):
        TrainImagePrep.box_params(-1.0)
    with pytest.raises(ValueError):
        TrainImagePrep(image_size=(512, 256), device="cpu")
