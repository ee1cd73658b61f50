"""Generate tests/golden/train_image_prep.npz by running THE REFERENCE's own BaseDataset.blur_image (PIL's GaussianBlur)
and the random draws of BehaveDataset.get_item / BaseDataset.blur_image.

Run in the build container only (needs /root/reference and PIL):

    python tests/golden/make_train_image_golden.py

data/base_data.py imports cv2 and torchvision at module level; neither is installed and blur_image uses neither, so
stand-ins are put into sys.modules for the import (the mechanism make_render_golden.py uses).

The fixture holds arrays only: a seeded (48, 64, 3) image, what blur_image made of it for aug_blur in {0.002, 0.01, 0.05}
under np.random.seed(seed), the radius each call drew, and the flip / radius sequence of eight items drawn in
get_item's order (train_data.py:49 `np.random.rand() > 0.5`, then base_data.py:125 `np.random.uniform(0, aug_blur) * 255.`).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
AUG_BLUR = (0.002, 0.01, 0.05)
BLUR_SEEDS = (11, 12, 13)
DRAW_SEED, DRAW_AUG_BLUR, DRAW_N = 5, 0.01, 8


def load_reference():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1
    sys.modules["cv2"] = cv2
    tv, tt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tv.transforms = tt
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tt
    sys.path.insert(0, REF)
    from data.base_data import BaseDataset
    return BaseDataset


def main():
    BaseDataset = load_reference()
    out = {}
    img = np.random.RandomState(2025).randint(0, 256, (48, 64, 3)).astype(np.uint8)
    # smooth part: a blur of pure noise tends to the mean; a ramp with an edge keeps structure at the large radii
    img[8:40, 8:56] = (np.mgrid[0:32, 0:48][1] * 5)[..., None].astype(np.uint8)
    img[20:28, 24:40] = 255
    out["image"] = img
    blurred, radii = [], []
    for aug, seed in zip(AUG_BLUR, BLUR_SEEDS):
        ds = BaseDataset([], 1, 0, aug_blur=aug)
        np.random.seed(seed)
        blurred.append(ds.blur_image(img.copy()))
        np.random.seed(seed)
        radii.append(np.random.uniform(0, aug) * 255.)          # the draw blur_image made (base_data.py:125)
    out["aug_blur"], out["blur_seed"] = np.asarray(AUG_BLUR), np.asarray(BLUR_SEEDS)
    out["blurred"], out["radius"] = np.stack(blurred), np.asarray(radii)
    # no blur below the threshold: the image comes back as it is, nothing is drawn
    ds = BaseDataset([], 1, 0, aug_blur=0.0)
    assert ds.blur_image(img) is img
    # the draw sequence of eight items: get_item's flip (random_flip=True, phase 'train'), then load_rgb -> blur_image's radius
    np.random.seed(DRAW_SEED)
    flips, rad = [], []
    for _ in range(DRAW_N):
        flips.append(bool((np.random.rand() > 0.5) & True))                    # train_data.py:49
        rad.append(np.random.uniform(0, DRAW_AUG_BLUR) * 255.)                 # base_data.py:125
    out["draw_seed"], out["draw_aug_blur"] = np.int64(DRAW_SEED), np.float64(DRAW_AUG_BLUR)
    out["draw_flip"], out["draw_radius"] = np.asarray(flips), np.asarray(rad)
    path = os.path.join(HERE, "train_image_prep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", "radii", radii, "flips", flips)


if __name__ == "__main__":
    main()
