"""Network input of a TRAINING batch from the decoded images, on the device.

Counterpart of BehaveDataset.prepare_image_crop (/root/reference/data/train_data.py:134-149) on top of BaseDataset
(data/base_data.py:71-192) from the point where the RGB image and the two masks are decoded uint8 arrays: the crop of
`crop_size` px around the centre of the masks' bounding box at the image's native resolution, resize to the network
input, / 255, background masking, channel stacking -- and the two augmentations train_launch.py exposes: `--random_flip`
(horizontal mirror of RGB and both masks) and `--aug_blur` (PIL.ImageFilter.GaussianBlur on the RGB image with radius
U(0, aug_blur) * 255; the masks are never blurred).  All pixel work runs in libchore_hip.so (csrc/image_prep.hip:
chore_prep_blur_u8, chore_prep_train_compose, chore_prep_masks2bbox); the host draws the random numbers and does the few
scalar steps in numpy with the reference's expressions.

    prep = TrainImagePrep(image_size=(512, 512), crop_size=1200, random_flip=True, aug_blur=0.01, seed=0)
    out = prep.prepare(rgb_u8, person_u8, obj_u8)          # (B,H,W,3), (B,H,W), (B,H,W)
    model(images=out["images"], crop_center=out["crop_center"], **sampler.train_batch(...))

`out["flip"]` tells the caller which items were mirrored: the mirrored meshes and `flip_part_labels` of the targets (the
reference reads them from a second `_flip.npz`) stay the caller's.

Kept from the reference, quirks included:
  * the crop centre of a mirrored item is that of the UNMIRRORED masks (get_crop_center reads the masks again without the
    mirror, train_data.py:115-132), so a mirrored crop is not centred on the mirrored subject;
  * the draw order per item: flip first (`np.random.rand() > 0.5`, only in phase 'train'), then the radius
    (`np.random.uniform(0, aug_blur) * 255.`, only when aug_blur > 1e-6, in every phase);
  * both asserts of get_crop_center, the second of which compares the y centre with the image WIDTH.
The blur is PIL's, bit for bit (pinned by a fixture BaseDataset.blur_image wrote, tests/golden/train_image_prep.npz); the
mirror commutes with it exactly, so the compose kernel mirrors by index after the blur.  cv2's resize arithmetic is
restated (oracle/image_prep.py): parity with cv2 itself is UNPINNED, as for ImagePrep.
"""
import numpy as np
import torch

from .. import _lib
from .image_prep import ImagePrep


class TrainImagePrep:
    def __init__(self, image_size=(512, 512), crop_size=1200, phase="train", random_flip=False, aug_blur=0.0, seed=None,
                 device="cuda:0"):
        if phase not in ("train", "val", "test"):
            raise ValueError("phase is 'train', 'val' or 'test'")
        if image_size[0] != image_size[1]:
            raise ValueError("the crop is square: image_size must be (S, S)")
        self.img_size, self.crop_size = tuple(image_size), crop_size
        self.phase, self.random_flip, self.aug_blur = phase, bool(random_flip), float(aug_blur)
        self.rng = np.random.RandomState(seed)
        self.device = torch.device(device)
        self._bbox = ImagePrep(image_size=image_size, crop_size=crop_size, device=device)

    # ---- the host's scalar steps -----------------------------------------------------------------------------------
    @staticmethod
    def box_params(radius):
        """(R, ww, fw) of PIL's GaussianBlur(radius): integer part of the effective box radius, 24-bit weight of a whole pixel
        and of the two fractional end pixels; (0, 0, 0) = copy (radius 0).  PIL's C code holds the radius and every
        intermediate in float32 and evaluates only the sqrt and the floor in double; the weight's division is float32."""
        f = np.float32
        r = f(radius)
        if not np.isfinite(r) or r < 0:
            raise ValueError("the blur radius must be finite and >= 0")
        s2 = f(r * r) / f(3)
        L = f(np.sqrt(12.0 * float(s2) + 1.0))
        l = f(np.floor((float(L) - 1.0) / 2.0))
        a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * s2)))
        a = f(a / f(f(6) * f(s2 - f(f(l + f(1)) * f(l + f(1))))))
        fr = f(l + a)
        if fr == 0:
            return 0, 0, 0
        R = int(fr)
        ww = int(np.uint32(f(1 << 24) / (fr * f(2) + f(1))))
        return R, ww, ((1 << 24) - (2 * R + 1) * ww) // 2

    def draw(self, n, flip=None, blur_radius=None):
        """flip (n,) bool and blur_radius (n,) float64 of n items; values that are not given are drawn from the instance's
        RandomState in the reference's order (per item: flip, then radius) with its expressions"""
        flips, radii = np.zeros(n, bool), np.zeros(n, np.float64)
        for i in range(n):
            if flip is None:
                flips[i] = (self.rng.rand() > 0.5) & self.random_flip if self.phase == "train" else False
            if blur_radius is None and self.aug_blur > 0.000001:
                radii[i] = self.rng.uniform(0, self.aug_blur) * 255.
        if flip is not None:
            flips[:] = np.asarray(flip, bool).reshape(n)
        if blur_radius is not None:
            radii[:] = np.asarray(blur_radius, np.float64).reshape(n)
        return flips, radii

    def _params(self, radii):
        """-> (B,3) int32 numpy, largest R; ValueError above the kernel's cap"""
        prm = np.array([self.box_params(r) for r in radii], np.int64).reshape(-1, 3)
        cap = int(_lib.lib.chore_prep_blur_max_radius())
        if prm[:, 0].max() > cap:
            raise ValueError("blur radius {:.2f} gives a box radius of {}, above the supported {}".format(
                float(np.max(radii)), int(prm[:, 0].max()), cap))
        return prm.astype(np.int32), int(prm[:, 0].max())

    def _u8(self, a, ndim):
        if isinstance(a, (list, tuple)):
            a = torch.stack([torch.as_tensor(x) for x in a]) if isinstance(a[0], torch.Tensor) else np.stack(a)
        t = torch.as_tensor(a)
        if t.dtype != torch.uint8 or t.dim() != ndim:
            raise ValueError(f"expected a uint8 array with {ndim} dimensions")
        return t.to(self.device).contiguous()

    def _call(self):
        return _lib.handle(self.device.index or 0), torch.cuda.current_stream(self.device).cuda_stream

    # ---- the kernels ---------------------------------------------------------------------------------------------------
    def blur_workspace(self, shape):
        """the uint8 workspace of `blur` for images of `shape` = (B,H,W,C)"""
        B, H, W, C = shape
        return torch.empty(int(_lib.lib.chore_prep_blur_workspace_bytes(B, H, W, C)), dtype=torch.uint8, device=self.device)

    def blur(self, imgs, params, max_r, out=None, workspace=None):
        """PIL's GaussianBlur on imgs (B,H,W,C) uint8 on the device with params (B,3) int32 on the device (box_params per image).
        With `out` and `workspace` given nothing is allocated and nothing read back: the call records into a graph."""
        if imgs.dtype != torch.uint8 or imgs.dim() != 4 or params.dtype != torch.int32 or tuple(params.shape) != (imgs.shape[0], 3):
            raise ValueError("blur: imgs (B,H,W,C) uint8, params (B,3) int32")
        B, H, W, C = imgs.shape
        out = torch.empty_like(imgs) if out is None else out
        workspace = self.blur_workspace(imgs.shape) if workspace is None else workspace
        h, s = self._call()
        _lib.check(_lib.lib.chore_prep_blur_u8(h, imgs.data_ptr(), B, H, W, C, params.data_ptr(), int(max_r), out.data_ptr(),
                                               workspace.data_ptr(), s), h, "chore_prep_blur_u8")
        return out

    def compose(self, rgb, pm, om, tlbr, flip, out=None):
        """crop (corners tlbr (B,4) host ints), mirror (flip (B,) host), resize, / 255, compose -> (B,5,S,S) fp32"""
        for t, nd in ((rgb, 4), (pm, 3), (om, 3)):
            if t.dtype != torch.uint8 or t.dim() != nd:
                raise ValueError("compose: rgb (B,H,W,3), masks (B,H,W), uint8")
        B, H, W = pm.shape
        if tuple(rgb.shape) != (B, H, W, 3) or om.shape != pm.shape:
            raise ValueError("compose: the images of a batch have one size")
        S = self.img_size[0]
        out = torch.empty(B, 5, S, S, dtype=torch.float32, device=self.device) if out is None else out
        tlbr = np.ascontiguousarray(tlbr, dtype=np.int32).reshape(B, 4)
        flip = np.ascontiguousarray(flip, dtype=np.int32).reshape(B)
        h, s = self._call()
        _lib.check(_lib.lib.chore_prep_train_compose(h, rgb.data_ptr(), pm.data_ptr(), om.data_ptr(), B, H, W, tlbr.ctypes.data,
                                                     flip.ctypes.data, S, out.data_ptr(), s), h, "chore_prep_train_compose")
        return out

    def crop_corners(self, centers):
        """BaseDataset.crop's corners (base_data.py:141-142) for centres (B,2) -> (B,4) int"""
        size = np.array([self.crop_size, self.crop_size])
        c = np.asarray(centers)
        return np.concatenate([np.round(c - size / 2).astype(int), np.round(c + size / 2).astype(int)], 1)

    # ---- the loader's steps ----------------------------------------------------------------------------------------------
    def prepare(self, rgb, person_mask, obj_mask, flip=None, blur_radius=None):
        """rgb (B,H,W,3), masks (B,H,W): uint8 arrays of one size (numpy, torch, or lists of single images) ->
        dict(images (B,5,S,S) fp32 and crop_center (B,2) fp32 on the device, flip (B,) bool and blur_radius (B,) float64
        on the host).  `flip` / `blur_radius` given are used as they are; otherwise they are drawn (see `draw`).
        The crop centre is that of the UNMIRRORED masks also for a mirrored item, like the reference."""
        rgb, pm, om = self._u8(rgb, 4), self._u8(person_mask, 3), self._u8(obj_mask, 3)
        B = rgb.shape[0]
        if pm.shape[0] != B or om.shape[0] != B:
            raise ValueError("rgb and the masks hold one batch")
        flips, radii = self.draw(B, flip, blur_radius)
        prm, max_r = self._params(radii)
        centers = np.stack([self.get_crop_center(pm[b], om[b]) for b in range(B)])
        if prm[:, 1].any():
            rgb = self.blur(rgb, torch.from_numpy(prm).to(self.device), max_r)
        images = self.compose(rgb, pm, om, self.crop_corners(centers), flips)
        return dict(images=images, crop_center=torch.from_numpy(centers.astype(np.float32)).to(self.device), flip=flips,
                    blur_radius=radii)

    def get_crop_center(self, person_mask, obj_mask):
        """centre of the bounding box of both masks, as they are given (train_data.py:115-132) -> (2,) int"""
        bmin, bmax = self._bbox.masks2bbox([person_mask, obj_mask])
        crop_center = (bmin + bmax) // 2
        assert np.sum(crop_center > 0) == 2, 'invalid bbox found'
        iw = person_mask.shape[1]
        assert crop_center[0] < iw and crop_center[0] > 0, 'invalid crop center value {}'.format(crop_center)
        assert crop_center[1] < iw and crop_center[1] > 0, 'invalid crop center value {}'.format(crop_center)   # iw: the reference's
        return crop_center

    def blur_image(self, img, radius=None):
        """BaseDataset.blur_image on one decoded (H,W) or (H,W,3) uint8 image -> numpy; the radius is drawn when not given
        (and the image returned as it is when aug_blur is off)"""
        if radius is None:
            if not self.aug_blur > 0.000001:
                return np.asarray(img)
            radius = self.rng.uniform(0, self.aug_blur) * 255.
        t = torch.as_tensor(img)
        if t.dim() not in (2, 3):
            raise ValueError("expected an (H,W) or (H,W,C) image")
        x = self._u8(t, t.dim())
        prm, max_r = self._params([radius])
        if not prm[0, 1]:
            return x.cpu().numpy()
        out = self.blur(x.reshape(1, x.shape[0], x.shape[1], -1), torch.from_numpy(prm).to(self.device), max_r)
        return out.reshape(x.shape).cpu().numpy()

    def flip_image(self, img):
        """horizontal mirror of one decoded image -> numpy (base_data.py:89-93)"""
        return np.ascontiguousarray(np.asarray(img)[:, ::-1])

    def prepare_image_crop(self, rgb, person_mask, obj_mask, flip):
        """the reference's method on one item's decoded images -> ((5,S,S) numpy float32, crop_center (2,) int)"""
        out = self.prepare(torch.as_tensor(rgb)[None], torch.as_tensor(person_mask)[None], torch.as_tensor(obj_mask)[None],
                           flip=[bool(flip)])
        return out["images"][0].cpu().numpy(), out["crop_center"][0].cpu().numpy().astype(np.int64)
