"""Exact distance from points to a triangle mesh on the GPU (chore_mesh_dist_fwd, csrc/mesh_dist.hip), and the side of the
surface by the generalized winding number (chore_mesh_sdf_fwd, the same kernels with one more sum in the loop).

What the reference's sampler gets from `np.abs(igl.signed_distance(P, V, F)[0])`, its `I` and `C`, and from
`trimesh.proximity.ProximityQuery(mesh).vertex(P)[1]` (preprocess/boundary_sampler.py:45-64 of the reference).  Forward only:
nothing in the reference differentiates through it, the inputs are detached."""
import torch

from .. import _lib

UNSIGNED = ("dist", "face_idx", "closest", "vert_idx")
SIGNED = ("winding", "inside", "signed")
WANT = UNSIGNED + SIGNED
SIGN_MODES = ("inside", "winding")


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
    chore_mesh_sdf_fwd, whose first four outputs have the same bits.  Forward only."""
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
    p = points.detach().to(torch.float32)
    v = verts.detach().to(torch.float32)
    p = (p[None] if p.dim() == 2 else p).contiguous()
    v = (v[None] if v.dim() == 2 else v).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    if p.dim() != 3 or p.shape[-1] != 3 or v.dim() != 3 or v.shape[-1] != 3 or f.dim() != 2 or f.shape[-1] != 3:
        raise ValueError("mesh_distance: expected points (B,N,3), verts (B,V,3), faces (F,3)")
    if v.shape[0] != p.shape[0]:
        raise ValueError(f"mesh_distance: {p.shape[0]} point sets against {v.shape[0]} vertex sets")
    B, N, V, F = p.shape[0], p.shape[1], v.shape[1], f.shape[0]
    nbytes = (_lib.lib.chore_mesh_sdf_workspace_bytes if signed_call else _lib.lib.chore_mesh_dist_workspace_bytes)(B, N, V, F)
    if nbytes == 0:
        raise ValueError(f"mesh_distance: unsupported shape B={B} N={N} V={V} F={F}")
    h = _lib.handle(dev.index or 0)
    out = {"dist": torch.empty((B, N), dtype=torch.float32, device=dev)}
    if "face_idx" in names:
        out["face_idx"] = torch.empty((B, N), dtype=torch.int32, device=dev)
    if "closest" in names:
        out["closest"] = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    if "vert_idx" in names:
        out["vert_idx"] = torch.empty((B, N), dtype=torch.int32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None     # noqa: E731
    if signed_call:
        w = out["winding"] = torch.empty((B, N), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib.chore_mesh_sdf_fwd(h, p.data_ptr(), v.data_ptr(), f.data_ptr(), B, N, V, F, out["dist"].data_ptr(),
                                               ptr("face_idx"), ptr("closest"), ptr("vert_idx"), w.data_ptr(), ws.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), h, "chore_mesh_sdf_fwd")
        if "inside" in names or ("signed" in names and sign_mode == "inside"):
            out["inside"] = w.abs() > 0.5
        if "signed" in names:
            out["signed"] = torch.where(out["inside"], -out["dist"], out["dist"]) if sign_mode == "inside" else \
                (1.0 - 2.0 * w) * out["dist"]
    else:
        _lib.check(_lib.lib.chore_mesh_dist_fwd(h, p.data_ptr(), v.data_ptr(), f.data_ptr(), B, N, V, F, out["dist"].data_ptr(),
                                                ptr("face_idx"), ptr("closest"), ptr("vert_idx"), ws.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), h, "chore_mesh_dist_fwd")
    res = tuple(out[n][0] if unbatched else out[n] for n in names)
    return res[0] if single else res
