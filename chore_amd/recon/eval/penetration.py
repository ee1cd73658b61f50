"""How much of one fitted mesh sits inside another: the quantity the interpenetration term of the joint fit
(csrc/collision.hip) exists to drive down, measured independently of that term.

A vertex of B is inside A when |generalized winding number of A about it| > 0.5 (chore_amd.preprocess.mesh_distance,
`inside`); its depth is the exact distance to A's surface.  Both come from ONE mesh_distance call over the whole batch; no
host loop over frames.  Only A, the mesh that is tested against, has to be closed (`is_closed`): B's faces are not used.

`penetration` is the report (no gradient); `penetration_loss` is the same quantity as one differentiable number per frame, the
opt-in term of the joint fit (ReconFitterBase.PENETRATION_TERM)."""
import numpy as np
import torch

from ...preprocess.mesh_distance import mesh_distance


def is_closed(faces):
    """host, once per topology: True when every edge of the (F,3) faces is used exactly twice, in opposite directions
    (a consistently oriented surface without boundary)"""
    f = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces).astype(np.int64).reshape(-1, 3)
    if len(f) == 0:
        return False
    i, j = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]), np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    if (i == j).any() or i.min() < 0:
        return False
    m = int(max(i.max(), j.max())) + 1
    fwd, bwd = np.sort(i * m + j), np.sort(j * m + i)
    return bool((fwd[1:] != fwd[:-1]).all() and np.array_equal(fwd, bwd))      # no directed edge twice, each one's reverse once


def penetration(verts_a, faces_a, verts_b, faces_b=None):
    """vertices of B inside A, per frame.  verts_a (B,Va,3), verts_b (B,Vb,3) float tensors on the GPU (unbatched: (V,3)),
    faces_a (Fa,3) shared by the batch; faces_b is accepted for symmetry and not used -> dict of (B,) tensors on the device:
      count      int64    vertices of B inside A
      frac       float32  count / Vb
      max_depth  float32  largest distance of an inside vertex to A's surface (0 if there is none)
      mean_depth float32  mean of that distance over the inside vertices (0 if there is none)"""
    va = verts_a[None] if verts_a.dim() == 2 else verts_a
    vb = verts_b[None] if verts_b.dim() == 2 else verts_b
    dist, inside = mesh_distance(vb, va, faces_a, ("dist", "inside"))
    depth = torch.where(inside, dist, torch.zeros_like(dist))
    count = inside.sum(1)
    return {"count": count, "frac": count.to(torch.float32) / vb.shape[1], "max_depth": depth.max(1).values,
            "mean_depth": depth.sum(1) / count.clamp(min=1).to(torch.float32)}


def penetration_loss(verts_a, faces_a, verts_b):
    """the mean over ALL vertices of B of their depth inside A, per frame: sum_i inside_i dist_i / Vb -> (B,) float32 on the
    device (unbatched input: (1,)), = frac * mean_depth of penetration().  Differentiable in both vertex sets through the
    exact distance (chore_mesh_dist_bwd); `inside` is a constant of the step (the winding number is not differentiated).
    One mesh_distance call; nothing is read on the host, so a step that holds it can be captured into a graph."""
    va = verts_a[None] if verts_a.dim() == 2 else verts_a
    vb = verts_b[None] if verts_b.dim() == 2 else verts_b
    dist, inside = mesh_distance(vb, va, faces_a, ("dist", "inside"))
    return torch.where(inside, dist, torch.zeros_like(dist)).sum(1) / vb.shape[1]
