"""How much of the fitted object the fitted body hides, and the other way round: the visible fraction by which the reference
decides whether a frame counts (recon/evaluate.py:53-58, data/data_paths.py:63-71: sum(obj_rend_mask) / sum(obj_rend_full) < 0.30
skips the frame).  The reference reads it from mask files of the dataset; here it comes from the meshes themselves, so a fit of
an image without such files has it too.  The companion of recon/eval/penetration.py.

One instances call (chore_instances_fwd) for the whole batch through the Kinect colour camera of
utils/render_utils.setup_renderer, WITHOUT anti-aliasing: a pixel is one sample, so every count is an integer.  No gradient."""
import math

import torch

MIN_VISIBLE = 0.30        # evaluate.py:57: a frame whose object is less visible than this is not evaluated
COUNT_KEYS = ("body_visible", "body_full", "object_visible", "object_full")


def occlusion(smpl_verts, smpl_faces, obj_verts, obj_faces, image_size=1024):
    """smpl_verts (B,Vs,3), obj_verts (B,Vo,3) float tensors on the GPU in camera coordinates (unbatched: (V,3)), smpl_faces
    (Fs,3), obj_faces (Fo,3) shared by the batch -> dict of (B,) tensors on the device:
      body_visible, object_visible  int64    pixels of the frame where the mesh is the nearest
      body_full, object_full        int64    pixels of the frame the mesh covers alone
      body_fraction, object_fraction float64 visible / full, NaN where full == 0
    The frame is the upper three quarters of the square rendering (the 2048 x 1536 frame: preprocess.masks.frame_rows)."""
    from ...preprocess.masks import frame_rows
    from ...utils.render_utils import setup_renderer
    if not smpl_verts.is_cuda or not obj_verts.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    sv = smpl_verts[None] if smpl_verts.dim() == 2 else smpl_verts
    ov = obj_verts[None] if obj_verts.dim() == 2 else obj_verts
    if sv.dim() != 3 or ov.dim() != 3 or sv.shape[0] != ov.shape[0] or sv.shape[2] != 3 or ov.shape[2] != 3:
        raise ValueError("smpl_verts (B,Vs,3) and obj_verts (B,Vo,3) of one batch size expected, got %s and %s"
                         % (tuple(smpl_verts.shape), tuple(obj_verts.shape)))
    dev, B = sv.device, sv.shape[0]
    rows = frame_rows(image_size)
    sf = torch.as_tensor(smpl_faces).to(dev).to(torch.int32).reshape(-1, 3)
    of = torch.as_tensor(obj_faces).to(dev).to(torch.int32).reshape(-1, 3)
    with torch.no_grad():
        verts = torch.cat((sv.detach().float(), ov.detach().float().to(dev)), dim=1)
        faces = torch.cat((sf, of + sv.shape[1]))[None].expand(B, -1, -1)
        group = torch.cat((torch.zeros(len(sf), dtype=torch.int32, device=dev),
                           torch.ones(len(of), dtype=torch.int32, device=dev)))[None].expand(B, -1)
        renderer = setup_renderer(image_size=image_size)
        renderer.anti_aliasing = False
        out = renderer.render_instances(verts, faces, group, 2)
        # at one sample per pixel the masks are 0 or 1: the sums are exact in int64
        vis = out["visible"][:, :, :rows].to(torch.int64).sum(dim=(2, 3))
        full = out["full"][:, :, :rows].to(torch.int64).sum(dim=(2, 3))
        frac = vis.double() / full.double()                   # 0 / 0 = NaN
    return {"body_visible": vis[:, 0], "body_full": full[:, 0], "object_visible": vis[:, 1], "object_full": full[:, 1],
            "body_fraction": frac[:, 0], "object_fraction": frac[:, 1]}


def frame_report(body_visible, body_full, object_visible, object_full):
    """one frame's counts (integers) -> what k{id}.occlusion.json holds: the counts, the two fractions (None where full == 0) and
    object_evaluated = object_fraction >= MIN_VISIBLE, the reference's rule for keeping the frame"""
    counts = dict(zip(COUNT_KEYS, (int(body_visible), int(body_full), int(object_visible), int(object_full))))
    fraction = lambda v, f: float(v) / float(f) if f else float("nan")      # noqa: E731
    body, obj = fraction(counts["body_visible"], counts["body_full"]), fraction(counts["object_visible"], counts["object_full"])
    rep = dict(counts)
    rep["body_fraction"] = None if math.isnan(body) else body
    rep["object_fraction"] = None if math.isnan(obj) else obj
    rep["object_evaluated"] = bool(obj >= MIN_VISIBLE)         # NaN: not evaluated
    return rep
