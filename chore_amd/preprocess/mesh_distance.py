"""Exact distance from points to a triangle mesh on the GPU (chore_mesh_dist_fwd, csrc/mesh_dist.hip), the side of the
surface by the generalized winding number (chore_mesh_sdf_fwd, the same kernels with one more sum in the loop), and the
gradient of the distance with respect to the points and the mesh vertices (chore_mesh_dist_bwd, csrc/mesh_dist_bwd.hip).

What the reference's sampler gets from `np.abs(igl.signed_distance(P, V, F)[0])`, its `I` and `C`, and from
`trimesh.proximity.ProximityQuery(mesh).vertex(P)[1]` (preprocess/boundary_sampler.py:45-64 of the reference).  Nothing in
the reference differentiates through it; the gradient is what a mesh-based loss term of the fit needs
(recon/eval/penetration.py, penetration_loss)."""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib

UNSIGNED = ("dist", "face_idx", "closest", "vert_idx")
SIGNED = ("winding", "inside", "signed")
WANT = UNSIGNED + SIGNED
SIGN_MODES = ("inside", "winding")


def _forward(p, v, f, signed_call, face_idx, closest, vert_idx):
    """the forward call on prepared tensors (detached, float32 / int32, contiguous, batched) -> dict of the outputs"""
    dev = p.device
    B, N, V, F = p.shape[0], p.shape[1], v.shape[1], f.shape[0]
    nbytes = (_lib.lib.chore_mesh_sdf_workspace_bytes if signed_call else _lib.lib.chore_mesh_dist_workspace_bytes)(B, N, V, F)
    if nbytes == 0:
        raise ValueError(f"mesh_distance: unsupported shape B={B} N={N} V={V} F={F}")
    h = _lib.handle(dev.index or 0)
    out = {"dist": torch.empty((B, N), dtype=torch.float32, device=dev)}
    if face_idx:
        out["face_idx"] = torch.empty((B, N), dtype=torch.int32, device=dev)
    if closest:
        out["closest"] = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    if vert_idx:
        out["vert_idx"] = torch.empty((B, N), dtype=torch.int32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None     # noqa: E731
    if signed_call:
        w = out["winding"] = torch.empty((B, N), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib.chore_mesh_sdf_fwd(h, p.data_ptr(), v.data_ptr(), f.data_ptr(), B, N, V, F, out["dist"].data_ptr(),
                                               ptr("face_idx"), ptr("closest"), ptr("vert_idx"), w.data_ptr(), ws.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), h, "chore_mesh_sdf_fwd")
    else:
        _lib.check(_lib.lib.chore_mesh_dist_fwd(h, p.data_ptr(), v.data_ptr(), f.data_ptr(), B, N, V, F, out["dist"].data_ptr(),
                                                ptr("face_idx"), ptr("closest"), ptr("vert_idx"), ws.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), h, "chore_mesh_dist_fwd")
    return out


class _MeshDistFn(torch.autograd.Function):
    """dist (differentiable in points and verts) + face_idx, closest, vert_idx / winding or None (no gradient).  The forward
    always asks for face_idx -- the backward reads the winner and forms its closest point again in fp64, so `closest` is computed
    only when the caller wants it; the optional outputs never change the others' bits."""

    @staticmethod
    def forward(ctx, points, verts, faces, signed_call, closest, vert_idx):
        p, v = points.detach(), verts.detach()
        out = _forward(p, v, faces, signed_call, True, closest, vert_idx)
        if _lib.lib.chore_mesh_dist_bwd_workspace_bytes(p.shape[0], p.shape[1], v.shape[1], faces.shape[0]) == 0:
            raise ValueError(f"mesh_distance: no gradient at shape B={p.shape[0]} N={p.shape[1]} V={v.shape[1]} F={faces.shape[0]}")
        ctx.save_for_backward(p, v, faces, out["face_idx"], out["dist"])
        res = (out["dist"], out["face_idx"], out.get("closest"), out.get("vert_idx"), out.get("winding"))
        ctx.mark_non_differentiable(*[t for t in res[1:] if t is not None])
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dist, *_):
        p, v, f, face_idx, dist = ctx.saved_tensors
        dev = p.device
        B, N, V, F = p.shape[0], p.shape[1], v.shape[1], f.shape[0]
        g = g_dist.to(torch.float32).contiguous()
        dp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        dv = torch.empty_like(v) if ctx.needs_input_grad[1] else None
        if dp is None and dv is None:
            return None, None, None, None, None, None
        ws = torch.empty(_lib.lib.chore_mesh_dist_bwd_workspace_bytes(B, N, V, F), dtype=torch.uint8, device=dev)
        h = _lib.handle(dev.index or 0)
        _lib.check(_lib.lib.chore_mesh_dist_bwd(h, p.data_ptr(), v.data_ptr(), f.data_ptr(), face_idx.data_ptr(), None,
                                                dist.data_ptr(), g.data_ptr(), B, N, V, F, None if dp is None else dp.data_ptr(),
                                                None if dv is None else dv.data_ptr(), ws.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), h, "chore_mesh_dist_bwd")
        return dp, dv, None, None, None, None


def mesh_distance(points, verts, faces, want=("dist",), sign_mode="inside"):
    """points (B,N,3) or (N,3), verts (B,V,3) or (V,3) float tensors on the GPU, faces (F,3) integer tensor shared by the batch.
    `want`: names out of dist (B,N) float32, face_idx (B,N) int32, closest (B,N,3) float32, vert_idx (B,N) int32 and
      winding (B,N) float32   the generalized winding number of the mesh about the point, the raw value: +1 inside a closed
                              mesh with outward faces, -1 with inward faces, 0 outside, fractional about an open mesh
      inside (B,N) bool       |winding| > 0.5.  The absolute value makes a closed mesh whose faces are consistently oriented
                              INWARD give the same answer as the outward one; about an open mesh it is the side on which
                              the surface covers more than half of the sphere of directions
      signed (B,N) float32    sign_mode="inside" (the default): -dist where inside, +dist elsewhere.
                              sign_mode="winding": (1 - 2 winding) dist, the fractional rule libigl's winding-number sign
                              type is SUPPOSED to apply -- unverified against igl (it is not available to this project);
                              off a watertight mesh its magnitude is not the distance
    -> a tuple of tensors in the order asked for (one tensor for a single name given as a string).  Unbatched input gives
    unbatched output.  Calls that ask only for the first four names run chore_mesh_dist_fwd; any of the last three runs
    chore_mesh_sdf_fwd, whose first four outputs have the same bits.

    Gradient: `dist`, and `signed` under sign_mode="inside" (the sign is a constant of the call: d signed = +-d dist), are
    differentiable with respect to `points` and `verts` whenever grad mode is on and one of the two requires grad
    (chore_mesh_dist_bwd: d dist / d p = (p - c) / dist, d dist / d corner k of the winning triangle = -b_k (p - c) / dist with
    b the barycentric coordinates of the closest point c; zero where dist == 0; first derivatives only).  The values are those
    of the plain call, bit for bit.  face_idx, closest, vert_idx, winding, inside, and signed under sign_mode="winding" stay
    detached: no gradient flows through the closest point or the winding number."""
    single = isinstance(want, str)
    names = (want,) if single else tuple(want)
    for n in names:
        if n not in WANT:
            raise ValueError(f"mesh_distance: unknown output {n!r} (one of {WANT})")
    if sign_mode not in SIGN_MODES:
        raise ValueError(f"mesh_distance: unknown sign_mode {sign_mode!r} (one of {SIGN_MODES})")
    signed_call = any(n in SIGNED for n in names)
    for name, t in (("points", points), ("verts", verts), ("faces", faces)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"mesh_distance: {name} must be a tensor on the GPU (chore_amd has no CPU path)")
    dev = points.device
    if verts.device != dev or faces.device != dev:
        raise RuntimeError("mesh_distance: points, verts and faces must be on one device")
    unbatched = points.dim() == 2
    grad = torch.is_grad_enabled() and (points.requires_grad or verts.requires_grad) and \
        ("dist" in names or ("signed" in names and sign_mode == "inside"))
    p = (points if grad else points.detach()).to(torch.float32)
    v = (verts if grad else verts.detach()).to(torch.float32)
    p = (p[None] if p.dim() == 2 else p).contiguous()
    v = (v[None] if v.dim() == 2 else v).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    if p.dim() != 3 or p.shape[-1] != 3 or v.dim() != 3 or v.shape[-1] != 3 or f.dim() != 2 or f.shape[-1] != 3:
        raise ValueError("mesh_distance: expected points (B,N,3), verts (B,V,3), faces (F,3)")
    if v.shape[0] != p.shape[0]:
        raise ValueError(f"mesh_distance: {p.shape[0]} point sets against {v.shape[0]} vertex sets")
    if grad:
        res = _MeshDistFn.apply(p, v, f, signed_call, "closest" in names, "vert_idx" in names)
        out = {k: t for k, t in zip(("dist", "face_idx", "closest", "vert_idx", "winding"), res) if t is not None}
    else:
        out = _forward(p, v, f, signed_call, "face_idx" in names, "closest" in names, "vert_idx" in names)
    if signed_call:
        w = out["winding"]
        if "inside" in names or ("signed" in names and sign_mode == "inside"):
            out["inside"] = w.abs() > 0.5
        if "signed" in names:       # sign_mode="winding" multiplies by the detached winding number and is itself detached
            out["signed"] = torch.where(out["inside"], -out["dist"], out["dist"]) if sign_mode == "inside" else \
                (1.0 - 2.0 * w) * out["dist"].detach()
    res = tuple(out[n][0] if unbatched else out[n] for n in names)
    return res[0] if single else res
