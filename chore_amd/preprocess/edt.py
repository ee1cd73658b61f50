"""Exact Euclidean distance transform on the GPU (chore_edt_sq, csrc/sil_targets.hip): scipy.ndimage.distance_transform_edt's
convention for 2-D images, computed in integers -- a column pass, then a row pass that takes the integer minimum of
(x - x')^2 + g^2 -- so the squared distances are exact and the float64 result is the correctly rounded sqrt of an integer."""
import ctypes

import torch

from .. import _lib


def edt_tiles():
    """(columns per block of the column pass, threads per block of the row pass, largest H / W) of chore_edt_sq"""
    c, r, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.lib.chore_edt_tiles(ctypes.byref(c), ctypes.byref(r), ctypes.byref(m))
    return c.value, r.value, m.value


def edt_sentinel(H, W):
    """what chore_edt_sq writes to every pixel of an image without a feature pixel"""
    return 2 * max(int(H), int(W)) ** 2


def edt_squared(feature):
    """feature (B,H,W) device tensor -> (B,H,W) int32: squared distance to the nearest pixel with feature != 0 of the same image
    (edt_sentinel(H, W) everywhere in an image that has none).  No host synchronisation."""
    if not feature.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    if feature.dim() != 3:
        raise ValueError("edt_squared: a (B,H,W) tensor expected, got %s" % (tuple(feature.shape),))
    dev = feature.device
    B, H, W = feature.shape
    f = (feature != 0).to(torch.uint8).contiguous()
    d2 = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    nws = _lib.lib.chore_edt_workspace_bytes(B, H, W)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
    h = _lib.handle(dev.index or 0)
    _lib.check(_lib.lib.chore_edt_sq(h, f.data_ptr(), B, H, W, d2.data_ptr(), ws.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream), h, "chore_edt_sq")
    return d2


def distance_transform_edt(mask, return_squared=False):
    """scipy.ndimage.distance_transform_edt for (H,W) or (B,H,W) device tensors: the distance from every non-zero pixel to the
    nearest zero pixel of its image, 0 at zero pixels.  float64 sqrt(d2), or the exact int32 squares with return_squared.
    An image without a zero pixel gets sqrt(2 max(H,W)^2) (edt_sentinel) everywhere: scipy's values in that case are an artefact
    of its implementation and are not reproduced.  H, W <= 4096."""
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    if mask.dim() not in (2, 3):
        raise ValueError("distance_transform_edt: (H,W) or (B,H,W) expected, got %s" % (tuple(mask.shape),))
    m = mask if mask.dim() == 3 else mask[None]
    d2 = edt_squared(m == 0)
    if not return_squared:
        dev = mask.device
        out = torch.empty(d2.shape, dtype=torch.float64, device=dev)
        h = _lib.handle(dev.index or 0)
        _lib.check(_lib.lib.chore_edt_sqrt_f64(h, d2.data_ptr(), d2.numel(), out.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), h, "chore_edt_sqrt_f64")
        d2 = out
    return d2 if mask.dim() == 3 else d2[0]
