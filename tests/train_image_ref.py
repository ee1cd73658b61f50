"""numpy references of the training image preparation (test helper, no test in here).

  pil_blur_ref    PIL.ImageFilter.GaussianBlur(radius) on a uint8 (H,W) or (H,W,C) image, restated: three box-blur passes
                  along the rows, then three along the columns, every pass rounded to uint8, channels independent.
                  Pinned against PIL itself by tests/test_train_image_host.py and against BaseDataset.blur_image by the
                  fixture tests/golden/train_image_prep.npz.
  train_crop_ref  BehaveDataset.prepare_image_crop (data/train_data.py:134-149) from decoded images: mirror, blur, crop
                  around a given centre, resize, / 255, compose -- oracle.image_prep's crop / resize_linear_u8 and the
                  compose expression of base_data.py:178-192 (cv2's resize is restated there: parity UNPINNED at cv2).
"""
import numpy as np

from oracle import image_prep as oi


def box_params_ref(radius):
    """(fr, R, ww, fw): effective box radius as float32, its integer part, the 24-bit weight of a full pixel and of the
    two fractional end pixels"""
    # PIL's C code holds the radius and every intermediate in float32 variables; only the sqrt and the floor are
    # evaluated in double.  (With all of it in double, radius 0.78817007 gives a weight one unit of 2^-24 off and an image
    # one grey level off PIL's; in float32 2300 radii in [0, 45] all match.)
    f = np.float32
    r = f(radius)
    s2 = f(r * r) / f(3)
    L = f(np.sqrt(12.0 * float(s2) + 1.0))
    l = f(np.floor((float(L) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * s2)))
    a = f(a / f(f(6) * f(s2 - f(f(l + f(1)) * f(l + f(1))))))
    fr = f(l + a)
    if fr == 0:
        return fr, 0, 0, 0
    R = int(fr)
    ww = int(np.uint32(np.float32(1 << 24) / (fr * np.float32(2) + np.float32(1))))      # the division is float32
    fw = ((1 << 24) - (2 * R + 1) * ww) // 2
    return fr, R, ww, fw


def _box_pass(p, R, ww, fw, axis):
    """one pass along `axis` of a uint32 array: out[x] = (ww * sum_{|k| <= R} p[x + k] + fw * (p[x - R - 1] + p[x + R + 1])
    + 2^23) >> 24 with the ends replicated; the weights add to at most 2^24, so uint32 holds every term"""
    n = p.shape[axis]
    pad = [(0, 0)] * p.ndim
    pad[axis] = (R + 1, R + 1)
    e = np.pad(p, pad, mode="edge")                                    # e[i] = p[clip(i - R - 1)]
    pad[axis] = (1, 0)
    c = np.pad(np.cumsum(e, axis=axis, dtype=np.uint32), pad)          # c[i] = e[0] + .. + e[i - 1]

    def sl(a, start):
        return np.take(a, np.arange(start, start + n), axis=axis)
    acc = sl(c, 2 * R + 2) - sl(c, 1)
    ends = sl(e, 0) + sl(e, 2 * R + 2)
    return (np.uint32(ww) * acc + np.uint32(fw) * ends + np.uint32(1 << 23)) >> np.uint32(24)


def pil_blur_ref(img, radius):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    fr, R, ww, fw = box_params_ref(radius)
    if fr == 0:
        return img.copy()
    p = img.astype(np.uint32)
    for axis in (1, 0):
        for _ in range(3):
            p = _box_pass(p, R, ww, fw, axis)
    assert p.max() <= 255
    return p.astype(np.uint8)


def train_crop_ref(rgb, person_mask, obj_mask, center, flip, radius, img_size, crop_size):
    """-> (5,S,S) float32.  `center` is the crop centre of the UNFLIPPED masks (get_crop_center reads them again without
    the mirror), `radius` the PIL radius of the blur (0: none); the masks are never blurred"""
    if flip:
        rgb, person_mask, obj_mask = rgb[:, ::-1], person_mask[:, ::-1], obj_mask[:, ::-1]
    rgb = pil_blur_ref(np.ascontiguousarray(rgb), radius)
    cs = np.array([crop_size, crop_size])
    center = np.asarray(center)
    rgb = oi.resize_linear_u8(oi.crop(rgb, center, cs), img_size) / 255.
    person_mask = oi.resize_linear_u8(oi.crop(np.ascontiguousarray(person_mask), center, cs), img_size) / 255.
    obj_mask = oi.resize_linear_u8(oi.crop(np.ascontiguousarray(obj_mask), center, cs), img_size) / 255.
    mask_comb = (person_mask > 0.5) | (obj_mask > 0.5)
    rgb = rgb * np.expand_dims(mask_comb, -1)
    images = np.dstack((rgb, person_mask, obj_mask))
    return images.transpose((2, 0, 1)).astype(np.float32)
