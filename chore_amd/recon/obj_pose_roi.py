"""Occlusion-aware silhouette loss on a region of interest, rendered by the HIP rasteriser.

Counterpart of /root/reference/recon/obj_pose_roi.py (SilLossROI) and of the pieces of the vendored
neural_renderer it drives (external/neural_renderer/neural_renderer/: projection.py:6-43, vertices_to_faces.py,
renderer.py:119-152 render_silhouettes, rasterize.py rasterize_silhouettes).  The rasterisation -- forward and the
edge-walk backward -- runs in libchore_hip.so (chore_silhouette_fwd / _bwd); object placement, camera projection and the
triangle list are one launch each way (chore_sil_project_fwd / _bwd; `projection` / `vertices_to_faces` below are the tensor
expressions of the reference, kept for its other callers and as what the tests compare with, `CHORE_SIL_TORCH_PROJECT=1`).

`SilLossROI.forward(R, obj_t, obj_s)` returns what the reference returns: `(loss_dict, image, edges, image_ref,
edt_ref_edge)` with `loss_dict["mask"] = mean_b sum_pixels (keep_mask * silhouette - image_ref)^2`.

Constructor: the reference crops the person / object masks to an expanded square box around the object mask with
detectron2's BitMasks.crop_and_resize and builds the ROI intrinsics from the Kinect calibration
(obj_pose_roi.py:21-98,125-142).  detectron2 / cv2 are not available here; the same steps are restated with numpy
/ torch (bounding box of the mask, PHOSA's make_bbox_square, bilinear crop sampled at pixel centres, threshold 0.5).
That preprocessing is setup code outside the fitting loop and its parity with detectron2 is NOT pinned; callers
that already own the cropped masks can pass them with `SilLossROI.from_crops`.

`SilLossROI.from_masks` / `set_masks` do the constructor's work on the device without a host round trip (csrc/sil_targets.hip:
chore_sil_targets, chore_sil_edge_edt), so a kept fitting chain refreshes its term inside recorded graphs; `edge_loss` is
PHOSA's edge term on `edt_ref_edge` (chore_sil_edge_fwd / _bwd), an opt-in term of the 'sil' phase that the reference does not have.

`set_occluder` / `depth_loss` are PHOSA's ordinal depth term (csrc/ordinal_depth.hip), opt-in as well: the body's depth image over
the ROI cameras is a constant of the call (the body is not stepped, it gets no gradient), the object's depth comes from the
winner map the mask term computes anyway (`mask_loss(parts=True)`).  A pixel the crops label as person AND object counts as
object, as for the mask term (cvt_masks) -- PHOSA's `mask_i & ~mask_j` would drop it from the object's side too.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib

NEAR, FAR, EPS = 0.1, 100.0, 1e-4   # rasterize.py:10-12 (rasterize_silhouettes is called with the defaults)


class _RasterizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tri, size):
        if not tri.is_cuda:
            raise RuntimeError("chore_amd needs device tensors (no CPU path)")
        dev = tri.device
        h = _lib.handle(dev.index or 0)
        B, Fn = tri.shape[:2]
        t = tri.detach().float().contiguous()
        fim = torch.empty(B, size, size, dtype=torch.int32, device=dev)
        alpha = torch.empty(B, size, size, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.lib.chore_silhouette_workspace_bytes(B, Fn), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.chore_silhouette_fwd(h, t.data_ptr(), B, Fn, size, NEAR, FAR, fim.data_ptr(), alpha.data_ptr(),
                                                 ws.data_ptr(), stream), h, "chore_silhouette_fwd")
        ctx.save_for_backward(t, fim, alpha)
        ctx.size = size
        ctx.mark_non_differentiable(fim)
        return alpha.clone(), fim

    @staticmethod
    def backward(ctx, g_alpha, _g_fim):
        t, fim, alpha = ctx.saved_tensors
        dev = t.device
        h = _lib.handle(dev.index or 0)
        B, Fn = t.shape[:2]
        g = torch.zeros_like(alpha) if g_alpha is None else g_alpha.float().contiguous()
        gt = torch.empty_like(t)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.chore_silhouette_bwd(h, t.data_ptr(), fim.data_ptr(), alpha.data_ptr(), g.data_ptr(), B, Fn,
                                                 ctx.size, EPS, gt.data_ptr(), stream), h, "chore_silhouette_bwd")
        return gt, None


class _PlacedTrianglesFn(torch.autograd.Function):
    """object pose -> the rasteriser's (B,2F,3,3) triangle list in one launch each way (chore_sil_project_fwd / _bwd):
    apply_transformation, projection, vertices_to_faces with both windings.  Gradients for R, obj_t, obj_s."""

    @staticmethod
    def forward(ctx, R, obj_t, obj_s, verts, faces32, K, cam_R, cam_t, adj_off, adj):
        dev = verts.device
        h = _lib.handle(dev.index or 0)
        R, obj_t, obj_s = R.float().contiguous(), obj_t.float().contiguous(), obj_s.float().contiguous()
        B, V, _ = verts.shape
        Fn = faces32.shape[1]
        tri = torch.empty(B, 2 * Fn, 3, 3, device=dev, dtype=torch.float32)
        bc = 1 if cam_R.shape[0] == 1 else 0
        _lib.check(_lib.lib.chore_sil_project_fwd(h, verts.data_ptr(), faces32.data_ptr(), R.data_ptr(), obj_t.data_ptr(),
                                                  obj_s.data_ptr(), K.data_ptr(), cam_R.data_ptr(), cam_t.data_ptr(), bc, None, 1.0,
                                                  1e-9, B, V, Fn, tri.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), h,
                   "chore_sil_project_fwd")
        ctx.save_for_backward(R, obj_t, obj_s, verts, K, cam_R, cam_t, adj_off, adj)
        ctx.dims = (B, V, Fn, bc)
        return tri

    @staticmethod
    def backward(ctx, g):
        R, obj_t, obj_s, verts, K, cam_R, cam_t, adj_off, adj = ctx.saved_tensors
        dev = verts.device
        h = _lib.handle(dev.index or 0)
        B, V, Fn, bc = ctx.dims
        g = g.float().contiguous()
        dR, dt, ds = torch.empty_like(R), torch.empty_like(obj_t), torch.empty_like(obj_s)
        _lib.check(_lib.lib.chore_sil_project_bwd(h, verts.data_ptr(), R.data_ptr(), obj_t.data_ptr(), obj_s.data_ptr(), K.data_ptr(),
                                                  cam_R.data_ptr(), cam_t.data_ptr(), bc, None, 1.0, 1e-9, B, V, Fn, adj_off.data_ptr(),
                                                  adj.data_ptr(), g.data_ptr(), dR.data_ptr(), dt.data_ptr(), ds.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), h, "chore_sil_project_bwd")
        return (dR, dt, ds) + (None,) * 7


class _EdgeTermFn(torch.autograd.Function):
    """image, weight (B,S,S) -> (B) sums of (maxpool_k(image) - image) * weight; gradient for the image only"""

    @staticmethod
    def forward(ctx, image, weight, ksize):
        if not image.is_cuda:
            raise RuntimeError("chore_amd needs device tensors (no CPU path)")
        dev = image.device
        h = _lib.handle(dev.index or 0)
        img, w = image.detach().float().contiguous(), weight.detach().float().contiguous()
        B, S = img.shape[:2]
        if img.dim() != 3 or img.shape[2] != S or w.shape != img.shape:
            raise ValueError("edge term: (B,S,S) image and weight expected, got %s and %s" % (tuple(img.shape), tuple(w.shape)))
        sums = torch.empty(B, dtype=torch.float32, device=dev)
        arg = torch.empty(B, S, S, dtype=torch.int32, device=dev)
        ws = torch.empty(max(_lib.lib.chore_sil_edge_workspace_bytes(B, S), 1), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib.chore_sil_edge_fwd(h, img.data_ptr(), w.data_ptr(), B, S, ksize, sums.data_ptr(), arg.data_ptr(),
                                               ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), h, "chore_sil_edge_fwd")
        ctx.save_for_backward(w, arg)
        ctx.ksize = ksize
        return sums

    @staticmethod
    def backward(ctx, g):
        w, arg = ctx.saved_tensors
        dev = w.device
        h = _lib.handle(dev.index or 0)
        B, S = w.shape[:2]
        g = g.float().contiguous()
        gi = torch.empty_like(w)
        _lib.check(_lib.lib.chore_sil_edge_bwd(h, w.data_ptr(), arg.data_ptr(), g.data_ptr(), B, S, ctx.ksize, gi.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), h, "chore_sil_edge_bwd")
        return gi, None, None


DEPTH_CLAMP = 2.0       # PHOSA's clamp of the depth difference in the ordinal depth term


def ordinal_depth_counts(tri, face_index, occ_depth, image_ref, keep_mask, c=DEPTH_CLAMP):
    """chore_ordinal_depth_fwd on device tensors: (per-frame sums (B), coef (B,S,S), counts (B,4) int32: pixels in case A, in
    case B, in person-and-both, in object-and-both), then the contiguous float triangles and winner map it read.  No gradient; _OrdinalDepthFn and the depth-order report call it."""
    if not tri.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    dev = tri.device
    h = _lib.handle(dev.index or 0)
    t = tri.detach().float().contiguous()
    B, Fn = t.shape[:2]
    S = face_index.shape[1]
    fim = face_index.contiguous()
    maps = [m.detach().float().contiguous() for m in (occ_depth, image_ref, keep_mask)]
    if tuple(face_index.shape) != (B, S, S) or face_index.dtype != torch.int32 or any(tuple(m.shape) != (B, S, S) for m in maps):
        raise ValueError("ordinal depth term: (B,S,S) int32 face_index and (B,S,S) occluder depth and masks expected")
    sums = torch.empty(B, dtype=torch.float32, device=dev)
    coef = torch.empty(B, S, S, dtype=torch.float32, device=dev)
    counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
    ws = torch.empty(max(_lib.lib.chore_ordinal_depth_workspace_bytes(B, S), 1), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.chore_ordinal_depth_fwd(h, t.data_ptr(), fim.data_ptr(), maps[0].data_ptr(),
                                                maps[1].data_ptr(), maps[2].data_ptr(), B, Fn, S, FAR, float(c), sums.data_ptr(),
                                                coef.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), h, "chore_ordinal_depth_fwd")
    return sums, coef, counts, t, fim


class _OrdinalDepthFn(torch.autograd.Function):
    """tri (B,F,3,3) and the step's winner map -> (B) sums of the ordinal depth term against the constant occluder depth;
    gradient for the triangles only (it feeds _PlacedTrianglesFn's backward; the occluder and the masks get none)"""

    @staticmethod
    def forward(ctx, tri, face_index, occ_depth, image_ref, keep_mask, c):
        sums, coef, _, t, fim = ordinal_depth_counts(tri, face_index, occ_depth, image_ref, keep_mask, c)
        ctx.save_for_backward(t, fim, coef)
        return sums

    @staticmethod
    def backward(ctx, g):
        t, fim, coef = ctx.saved_tensors
        dev = t.device
        h = _lib.handle(dev.index or 0)
        B, Fn = t.shape[:2]
        g = g.float().contiguous()
        gt = torch.empty_like(t)
        _lib.check(_lib.lib.chore_ordinal_depth_bwd(h, t.data_ptr(), fim.data_ptr(), coef.data_ptr(), g.data_ptr(), B, Fn,
                                                    fim.shape[1], gt.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), h,
                   "chore_ordinal_depth_bwd")
        return gt, None, None, None, None, None


def corner_adjacency(faces, num_verts):
    """for every vertex the entries (f2 * 3 + corner) of the doubled face list (faces, then faces with reversed corners) that
    reference it, ascending: (offsets (V+1) int32, entries int32)"""
    f = np.asarray(faces, np.int64)
    both = np.concatenate([f, f[:, ::-1]], 0).reshape(-1)           # entry e = f2 * 3 + corner -> vertex
    order = np.argsort(both, kind="stable")
    counts = np.bincount(both, minlength=num_verts)
    off = np.zeros(num_verts + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return off.astype(np.int32), order.astype(np.int32)


def projection(vertices, K, R, t, dist_coeffs=None, orig_size=1.0, eps=1e-9):
    """[X,Y,Z] -> [u, v in [-1,1], z]   (neural_renderer/projection.py:6-43, op for op)"""
    v = torch.matmul(vertices, R.transpose(2, 1)) + t
    x, y, z = v[:, :, 0], v[:, :, 1], v[:, :, 2]
    x_ = x / (z + eps)
    y_ = y / (z + eps)
    if dist_coeffs is None:
        dist_coeffs = torch.zeros(1, 5, device=vertices.device)
    k1, k2, p1, p2, k3 = (dist_coeffs[:, None, i] for i in range(5))
    r = torch.sqrt(x_ ** 2 + y_ ** 2)
    x__ = x_ * (1 + k1 * (r ** 2) + k2 * (r ** 4) + k3 * (r ** 6)) + 2 * p1 * x_ * y_ + p2 * (r ** 2 + 2 * x_ ** 2)
    y__ = y_ * (1 + k1 * (r ** 2) + k2 * (r ** 4) + k3 * (r ** 6)) + p1 * (r ** 2 + 2 * y_ ** 2) + 2 * p2 * x_ * y_
    h = torch.stack([x__, y__, torch.ones_like(z)], dim=-1)
    uv = torch.matmul(h, K.transpose(1, 2))
    u, vv = uv[:, :, 0], orig_size - uv[:, :, 1]
    u = 2 * (u - orig_size / 2.0) / orig_size
    vv = 2 * (vv - orig_size / 2.0) / orig_size
    return torch.stack([u, vv, z], dim=-1)


def vertices_to_faces(vertices, faces):
    """(B,V,3), (B,F,3) int -> (B,F,3,3)"""
    B, nv = vertices.shape[:2]
    idx = faces.long() + (torch.arange(B, device=vertices.device) * nv)[:, None, None]
    return vertices.reshape(B * nv, 3)[idx]


def render_silhouettes(vertices, faces, K, R, t, size, dist_coeffs=None, orig_size=1.0, fill_back=True):
    """nr.Renderer(camera_mode='projection', anti_aliasing=False)(vertices, faces, mode='silhouettes')
    (renderer.py:119-152): (B,size,size) images in {0,1}, differentiable w.r.t. the vertices"""
    if fill_back:
        faces = torch.cat((faces, faces.flip(-1)), dim=1)
    tri = vertices_to_faces(projection(vertices, K, R, t, dist_coeffs, orig_size), faces)
    alpha, _ = _RasterizeFn.apply(tri, size)
    return alpha.flip(1)          # rasterize_rgbad reverses the rows (rasterize.py:345)


# ---- mask preprocessing (setup, not on the fitting loop) ----------------------------------------------------
def mask2bbox(mask):
    """xyxy bounding box of mask > 0.5 (reference: cv2 contours of the thresholded mask, opt_utils.py:105-116)"""
    ys, xs = np.nonzero(np.asarray(mask) > 0.5)
    if ys.size == 0:
        raise ValueError("empty object mask")
    return np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float64)


def make_bbox_square(bbox_xywh, expansion=0.0):
    """PHOSA's square box around an xywh box (recon/bbox.py:25-46)"""
    b = np.asarray(bbox_xywh, np.float64).reshape(-1, 4)
    c = np.stack((b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2), 1)
    s = np.maximum(b[:, 2], b[:, 3])[:, None] * (1 + expansion)
    return np.hstack((c - s / 2, s, s)).reshape(np.asarray(bbox_xywh).shape)


def crop_and_resize(masks, boxes_xyxy, size):
    """bilinear crop of (B,H,W) masks to (B,size,size) sampled at the pixel centres of the output grid, then
    thresholded at 0.5 (what detectron2's BitMasks.crop_and_resize computes with roi_align(aligned=True))"""
    B, H, W = masks.shape
    out = []
    for m, bx in zip(masks.float(), boxes_xyxy):
        x0, y0, x1, y1 = [float(v) for v in bx]
        xs = x0 + (torch.arange(size, device=m.device, dtype=torch.float32) + 0.5) * (x1 - x0) / size - 0.5
        ys = y0 + (torch.arange(size, device=m.device, dtype=torch.float32) + 0.5) * (y1 - y0) / size - 0.5
        gx = 2 * xs / max(W - 1, 1) - 1
        gy = 2 * ys / max(H - 1, 1) - 1
        grid = torch.stack(torch.meshgrid(gy, gx, indexing="ij")[::-1], -1)[None]
        out.append(F.grid_sample(m[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0])
    return torch.stack(out) >= 0.5


class SilLossROI(nn.Module):
    net_input_size = 512

    def __init__(self, person_masks, obj_masks, temp_mesh, crop_centers, rend_size=256, kernel_size=7,
                 bbox_expansion=0.3, device="cuda:0", crop_size=1200):
        """the reference's argument list (obj_pose_roi.py:21-29).  person_masks / obj_masks: (B,512,512) network-input
        masks; temp_mesh: the centred template, an object with .v (V,3) and .f (F,3) or a (verts, faces) pair;
        crop_centers (B,2) in original-image pixels"""
        super().__init__()
        dev = torch.device(device)
        temp_verts, temp_faces = (temp_mesh.v, temp_mesh.f) if hasattr(temp_mesh, "v") else temp_mesh
        person_masks, obj_masks = torch.as_tensor(person_masks).to(dev), torch.as_tensor(obj_masks).to(dev)
        boxes = np.stack([mask2bbox(m.cpu().numpy()) for m in obj_masks])                       # xyxy
        xywh = np.concatenate([boxes[:, :2], boxes[:, 2:] - boxes[:, :2]], 1)
        sq = make_bbox_square(xywh, bbox_expansion)                                             # xywh
        sq_xyxy = np.concatenate([sq[:, :2], sq[:, :2] + sq[:, 2:]], 1)
        obj_crop = crop_and_resize(obj_masks, sq_xyxy, rend_size)
        ps_crop = crop_and_resize(person_masks, sq_xyxy, rend_size)
        scale = crop_size / float(self.net_input_size)
        Ks = []
        cc = torch.as_tensor(crop_centers).float().cpu().numpy()
        for bbox, c in zip(sq, cc):
            Ks.append(self.compute_K_roi(self.to_original_bbox(bbox, scale, c, crop_size)))
        self._setup(obj_crop, ps_crop, torch.cat(Ks, 0).to(dev), temp_verts, temp_faces, rend_size, kernel_size, dev)

    @classmethod
    def from_crops(cls, obj_crop, person_crop, K_rois, temp_verts, temp_faces, kernel_size=7, device="cuda:0"):
        """build from already cropped (B,S,S) boolean masks and (B,3,3) ROI intrinsics"""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        dev = torch.device(device)
        obj_crop = torch.as_tensor(obj_crop).to(dev) > 0
        person_crop = torch.as_tensor(person_crop).to(dev) > 0
        self._setup(obj_crop, person_crop, torch.as_tensor(K_rois).float().to(dev), temp_verts, temp_faces,
                    obj_crop.shape[-1], kernel_size, dev)
        return self

    def _setup(self, obj_crop, ps_crop, Ks, temp_verts, temp_faces, rend_size, kernel_size, dev):
        B = obj_crop.shape[0]
        self.rend_size = rend_size
        self.register_buffer("image_ref", obj_crop.float())                    # edges / target: the object mask only
        self.register_buffer("keep_mask", self.cvt_masks(ps_crop, obj_crop).float())
        self.pool = nn.MaxPool2d(kernel_size=kernel_size, stride=1, padding=kernel_size // 2)
        self.prepare_dist_trans(self.image_ref)
        self.register_buffer("K", Ks)
        self._setup_template(temp_verts, temp_faces, B, dev)

    def _setup_template(self, temp_verts, temp_faces, B, dev):
        verts = torch.as_tensor(np.asarray(temp_verts), dtype=torch.float32)
        faces = torch.as_tensor(np.asarray(temp_faces).astype(np.int64))
        self.register_buffer("vertices", verts.repeat(B, 1, 1).to(dev))
        self.register_buffer("faces", faces.repeat(B, 1, 1).to(dev))
        self.register_buffer("R", torch.eye(3, device=dev).unsqueeze(0))
        self.register_buffer("t", torch.zeros(1, 3, device=dev))
        # for the one-launch placement + projection (_PlacedTrianglesFn): int32 faces and the corner lists of the vertices
        off, ent = corner_adjacency(faces.numpy(), verts.shape[0])
        self.register_buffer("faces32", self.faces.to(torch.int32).contiguous(), persistent=False)
        self.register_buffer("adj_off", torch.from_numpy(off).to(dev), persistent=False)
        self.register_buffer("adj", torch.from_numpy(ent).to(dev), persistent=False)

    @classmethod
    def from_masks(cls, person_masks, obj_masks, temp_mesh, crop_centers, rend_size=256, kernel_size=7, bbox_expansion=0.3,
                   device="cuda:0", crop_size=1200):
        """the constructor's arguments and buffers, filled on the device (chore_sil_targets, chore_sil_edge_edt) without a host
        synchronisation: nothing is downloaded, no device value is read on the host.  One more buffer, `valid` (B) int32, and
        `box_sq` (B,4) float64, the square boxes.  Differences from the constructor: the crops' coordinates and weights are
        computed in float64 (the constructor's grid_sample runs in float32, so a pixel whose value lies within float32 round-off
        of the 0.5 threshold can differ); and a frame whose object mask is EMPTY cannot raise ValueError as the constructor does,
        for that would need a synchronisation -- it gets valid = 0, all-zero image_ref and keep_mask (its mask term is 0) and the
        finite K of the whole image.  Check `valid` where an empty mask is an error."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("chore_amd needs device tensors (no CPU path)")
        temp_verts, temp_faces = (temp_mesh.v, temp_mesh.f) if hasattr(temp_mesh, "v") else temp_mesh
        obj_masks = torch.as_tensor(obj_masks)
        B, S = obj_masks.shape[0], int(rend_size)
        self.rend_size, self.kernel_size = S, int(kernel_size)
        self.bbox_expansion, self.crop_size = float(bbox_expansion), float(crop_size)
        self.pool = nn.MaxPool2d(kernel_size=kernel_size, stride=1, padding=kernel_size // 2)
        for name in ("image_ref", "keep_mask", "edt_ref_edge"):
            self.register_buffer(name, torch.empty(B, S, S, dtype=torch.float32, device=dev))
        self.register_buffer("K", torch.empty(B, 3, 3, dtype=torch.float32, device=dev))
        self.register_buffer("valid", torch.empty(B, dtype=torch.int32, device=dev))
        self.register_buffer("box_sq", torch.empty(B, 4, dtype=torch.float64, device=dev))
        # scratch of the two launches, kept: set_masks runs inside recorded graphs
        self.register_buffer("ref_edges", torch.empty(B, S, S, dtype=torch.float32, device=dev), persistent=False)
        nws = max(_lib.lib.chore_sil_targets_workspace_bytes(B), _lib.lib.chore_sil_edge_edt_workspace_bytes(B, S), 1)
        self.register_buffer("_targets_ws", torch.empty(nws, dtype=torch.uint8, device=dev), persistent=False)
        self._setup_template(temp_verts, temp_faces, B, dev)
        return self.set_masks(person_masks, obj_masks, crop_centers)

    @torch.no_grad()
    def set_masks(self, person_masks, obj_masks, crop_centers):
        """new masks (B,H,W) and crop centres (B,2) for an object built by from_masks: image_ref, keep_mask, K, valid, box_sq and
        edt_ref_edge are refreshed IN PLACE (a recorded fitting step keeps reading these buffers), no host synchronisation"""
        if not hasattr(self, "_targets_ws"):
            raise RuntimeError("SilLossROI.set_masks: only for objects built by SilLossROI.from_masks")
        dev = self.image_ref.device
        B, S = self.image_ref.shape[:2]
        prep = lambda a: torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
        person, obj, cc = prep(person_masks), prep(obj_masks), prep(crop_centers)
        if obj.dim() != 3 or obj.shape[0] != B or person.shape != obj.shape or tuple(cc.shape) != (B, 2):
            raise ValueError("SilLossROI.set_masks: (B,H,W) masks and (B,2) centres for B = %d expected, got %s, %s, %s"
                             % (B, tuple(person.shape), tuple(obj.shape), tuple(cc.shape)))
        h = _lib.handle(dev.index or 0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.chore_sil_targets(h, person.data_ptr(), obj.data_ptr(), cc.data_ptr(), B, obj.shape[1], obj.shape[2], S,
                                              self.bbox_expansion, self.crop_size, self.net_input_size, self.image_ref.data_ptr(),
                                              self.keep_mask.data_ptr(), self.K.data_ptr(), self.box_sq.data_ptr(),
                                              self.valid.data_ptr(), self._targets_ws.data_ptr(), stream), h, "chore_sil_targets")
        _lib.check(_lib.lib.chore_sil_edge_edt(h, self.image_ref.data_ptr(), B, S, self.kernel_size, 0.25, self.ref_edges.data_ptr(),
                                               self.edt_ref_edge.data_ptr(), self._targets_ws.data_ptr(), stream), h,
                   "chore_sil_edge_edt")
        return self

    @torch.no_grad()
    def load_from(self, other):
        """take over another instance's per-image data IN PLACE (reference and keep masks, ROI cameras, edge distance
        transform): a recorded fitting step keeps reading this object's buffers across loader batches
        (recon_fit_behave._FitSlot); the template (vertices, faces, corner lists) does not change"""
        names = ("image_ref", "keep_mask", "K", "edt_ref_edge")
        if hasattr(self, "occ_depth") and hasattr(other, "occ_depth"):       # the occluder of the ordinal depth term, when both have one
            names += ("occ_depth",)
        for name in names:
            mine, theirs = getattr(self, name), getattr(other, name)
            if mine.shape != theirs.shape:
                raise ValueError("SilLossROI.load_from: %s has another shape" % name)
            mine.copy_(theirs)
        if self.vertices.shape != other.vertices.shape or not torch.equal(self.vertices, other.vertices):
            raise ValueError("SilLossROI.load_from: another template")
        return self

    def prepare_dist_trans(self, image_refs, power=0.25):
        """distance transform of the reference edges (obj_pose_roi.py:92-103); debugging output of forward()"""
        from scipy.ndimage import distance_transform_edt
        edges = self.compute_edges(image_refs).cpu().numpy()
        edt = np.stack([distance_transform_edt(1 - (e > 0)) ** (power * 2) for e in edges])
        self.register_buffer("edt_ref_edge", torch.from_numpy(edt).float().to(image_refs.device))

    def compute_edges(self, silhouette):
        return self.pool(silhouette) - silhouette

    @staticmethod
    def to_original_bbox(bbox_square, scale, trans, crop_size=1200):
        b = np.array(bbox_square, np.float64)
        b *= scale
        b[:2] += np.asarray(trans, np.float64) - crop_size / 2.0
        return b

    @staticmethod
    def compute_K_roi(bbox_square, kinect_width=2048):
        """intrinsics of a camera that sees only the square box (obj_pose_roi.py:125-142)"""
        x, y, b, w = bbox_square
        if abs(b - w) > 1e-6:
            raise ValueError("the given bbox is not square")
        fx, fy = 979.7844 / kinect_width, 979.840 / kinect_width
        cx, cy = 1018.952 / kinect_width, 779.486 / kinect_width
        return torch.tensor([[[fx * kinect_width / b, 0, (cx * kinect_width - x) / b],
                              [0, fy * kinect_width / b, (cy * kinect_width - y) / b],
                              [0, 0, 1]]], dtype=torch.float32)

    @staticmethod
    def cvt_masks(person_mask, obj_mask):
        """1 where the rendering counts (object foreground or free background), 0 where a person occludes
        (obj_pose_roi.py:144-157)"""
        fore, ps = obj_mask > 0.5, person_mask > 0.5
        inv = -ps.float()
        inv[fore] = 1.0
        return inv >= 0

    def apply_transformation(self, R, obj_t, obj_s):
        verts = torch.bmm(self.vertices, R) + obj_t.unsqueeze(1)
        return obj_s.view(-1, 1, 1) * verts

    def render_parts(self, R, obj_t, obj_s):
        """what one placement and one rasterisation of the step give: (silhouettes (B,S,S) as render() returns them, the
        (B,2F,3,3) triangle list, the (B,S,S) int32 winner map of chore_silhouette_fwd, rows NOT flipped).  The mask term and
        the ordinal depth term of a step share them.  Device path only."""
        if not (R.is_cuda and self.vertices.is_cuda and tuple(obj_s.shape) == (self.vertices.shape[0],)):
            raise RuntimeError("SilLossROI.render_parts needs device tensors and one scale per frame (no CPU path)")
        tri = _PlacedTrianglesFn.apply(R, obj_t, obj_s, self.vertices, self.faces32, self.K, self.R, self.t, self.adj_off, self.adj)
        alpha, fim = _RasterizeFn.apply(tri, self.rend_size)
        return alpha.flip(1), tri, fim

    def render(self, R, obj_t, obj_s):
        """silhouettes (B,S,S) of the template under the pose: apply_transformation -> render_silhouettes"""
        if (not os.environ.get("CHORE_SIL_TORCH_PROJECT") and R.is_cuda and self.vertices.is_cuda and
                tuple(obj_s.shape) == (self.vertices.shape[0],)):
            return self.render_parts(R, obj_t, obj_s)[0]
        verts = self.apply_transformation(R, obj_t, obj_s)
        return render_silhouettes(verts, self.faces, self.K, self.R, self.t, self.rend_size)

    def mask_loss(self, R, obj_t, obj_s, parts=False):
        """forward()[0] without the outputs the fitting loop does not read (the edge image costs a max-pool per step).
        parts: also the step's triangle list and winner map (render_parts), for depth_loss: ({"mask": ...}, image, tri, face_index)"""
        if parts:
            rendered, tri, fim = self.render_parts(R, obj_t, obj_s)
        else:
            rendered = self.render(R, obj_t, obj_s)
        image = self.keep_mask * rendered
        loss = {"mask": torch.sum((image - self.image_ref) ** 2, dim=(1, 2)).mean()}
        return (loss, image, tri, fim) if parts else (loss, image)

    @torch.no_grad()
    def set_occluder(self, verts, faces):
        """the constant occluder of the ordinal depth term: (B,V,3) camera-space vertices (the body; they are placed with the
        identity pose, both windings) and an (F,3) face array -> the kept buffer `occ_depth` (B,S,S): the depth of the nearest
        face at every pixel of this term's ROI cameras, FAR where there is none, in the orientation of image_ref
        (chore_sil_project_fwd, chore_silhouette_fwd, chore_sil_depth).  Refreshed IN PLACE on later calls (a recorded step keeps
        reading the buffer); no host synchronisation.  The occluder gets no gradient: the object fit does not step the body."""
        dev = self.image_ref.device
        B, S = self.image_ref.shape[:2]
        v = torch.as_tensor(verts).detach().to(device=dev, dtype=torch.float32).contiguous()
        if v.dim() != 3 or v.shape[0] != B or v.shape[2] != 3:
            raise ValueError("SilLossROI.set_occluder: (B,V,3) vertices for B = %d expected, got %s" % (B, tuple(v.shape)))
        f32 = torch.as_tensor(faces).to(device=dev, dtype=torch.int32).reshape(-1, 3)
        Fn, V = f32.shape[0], v.shape[1]
        if not hasattr(self, "occ_depth"):
            self.register_buffer("occ_depth", torch.empty(B, S, S, dtype=torch.float32, device=dev))
            self.register_buffer("_occ_eye", torch.eye(3, device=dev).repeat(B, 1, 1), persistent=False)
            self.register_buffer("_occ_zero", torch.zeros(B, 3, device=dev), persistent=False)
            self.register_buffer("_occ_one", torch.ones(B, device=dev), persistent=False)
        if getattr(self, "_occ_faces", None) is None or tuple(self._occ_faces.shape) != (B, Fn, 3):      # scratch, once per face count
            self._occ_faces = torch.empty(B, Fn, 3, dtype=torch.int32, device=dev)
            self._occ_tri = torch.empty(B, 2 * Fn, 3, 3, dtype=torch.float32, device=dev)
            self._occ_fim = torch.empty(B, S, S, dtype=torch.int32, device=dev)
            self._occ_alpha = torch.empty(B, S, S, dtype=torch.float32, device=dev)
            self._occ_ws = torch.empty(max(_lib.lib.chore_silhouette_workspace_bytes(B, 2 * Fn), 1), dtype=torch.uint8, device=dev)
        self._occ_faces.copy_(f32.unsqueeze(0).expand(B, -1, -1))
        h = _lib.handle(dev.index or 0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        bc = 1 if self.R.shape[0] == 1 else 0
        _lib.check(_lib.lib.chore_sil_project_fwd(h, v.data_ptr(), self._occ_faces.data_ptr(), self._occ_eye.data_ptr(),
                                                  self._occ_zero.data_ptr(), self._occ_one.data_ptr(), self.K.data_ptr(),
                                                  self.R.data_ptr(), self.t.data_ptr(), bc, None, 1.0, 1e-9, B, V, Fn,
                                                  self._occ_tri.data_ptr(), stream), h, "chore_sil_project_fwd")
        _lib.check(_lib.lib.chore_silhouette_fwd(h, self._occ_tri.data_ptr(), B, 2 * Fn, S, NEAR, FAR, self._occ_fim.data_ptr(),
                                                 self._occ_alpha.data_ptr(), self._occ_ws.data_ptr(), stream), h, "chore_silhouette_fwd")
        _lib.check(_lib.lib.chore_sil_depth(h, self._occ_tri.data_ptr(), self._occ_fim.data_ptr(), B, 2 * Fn, S, FAR, 1,
                                            self.occ_depth.data_ptr(), stream), h, "chore_sil_depth")
        return self

    def depth_loss(self, tri, face_index):
        """PHOSA's ordinal depth term on the step's triangle list and winner map (render_parts / mask_loss(parts=True)) against
        the occluder of set_occluder: {"depth": mean_b sum_pixels log1p(exp(min(violation, 2)))} over the pixels whose two depths
        contradict the masks (person pixel: the object is in front of the body; object pixel: the body is in front of the
        object), one launch pair each way (chore_ordinal_depth_fwd / _bwd).  Not a term of the reference's fit."""
        if not hasattr(self, "occ_depth"):
            raise RuntimeError("SilLossROI.depth_loss: call set_occluder first")
        return {"depth": _OrdinalDepthFn.apply(tri, face_index, self.occ_depth, self.image_ref, self.keep_mask, DEPTH_CLAMP).mean()}

    @torch.no_grad()
    def depth_order_counts(self, R, obj_t, obj_s):
        """(B,4) int32 of the pose: pixels in case A (person pixel, object in front), in case B (object pixel, body in front),
        person pixels where both meshes project, object pixels where both do (chore_ordinal_depth_fwd's counts)"""
        if not hasattr(self, "occ_depth"):
            raise RuntimeError("SilLossROI.depth_order_counts: call set_occluder first")
        _, tri, fim = self.render_parts(R, obj_t, obj_s)
        return ordinal_depth_counts(tri, fim, self.occ_depth, self.image_ref, self.keep_mask)[2]

    def edge_loss(self, image):
        """PHOSA's edge term on the image mask_loss returns: {"edge": mean_b sum_pixels compute_edges(image) * edt_ref_edge},
        forward and backward in one launch pair each (chore_sil_edge_fwd / _bwd).  Not a term of the reference's fit."""
        k = self.pool.kernel_size
        return {"edge": _EdgeTermFn.apply(image, self.edt_ref_edge, k if isinstance(k, int) else k[0]).mean()}

    def forward(self, R, obj_t, obj_s):
        loss_dict, image = self.mask_loss(R, obj_t, obj_s)
        return loss_dict, image, self.compute_edges(image), self.image_ref, self.edt_ref_edge

    def compute_offscreen_loss(self, verts):
        """penalty for leaving the view frustum (obj_pose_roi.py:179-199)"""
        proj = projection(verts, self.K, self.R, self.t, None, 1.0)
        xy, z = proj[:, :, :2], proj[:, :, 2:]
        zeros = torch.zeros_like(z)
        return (torch.max(xy - 1, zeros).sum(dim=(1, 2)) + torch.max(-1 - xy, zeros).sum(dim=(1, 2)) +
                torch.max(-z, zeros).sum(dim=(1, 2)) + torch.max(z - FAR, zeros).sum(dim=(1, 2)))
