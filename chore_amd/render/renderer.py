"""Colour / depth / coverage renderer for looking at fitted meshes, on the HIP rasteriser (chore_render_fwd).

Counterpart of the vendored neural_renderer as the reference's visualisation uses it
(external/neural_renderer/neural_renderer/ of a CHORE checkout: renderer.py:11-63,237-283 Renderer / render, lighting.py,
look_at.py, perspective.py, get_points_from_angles.py, rasterize.py:267-348 rasterize_rgbad).  The camera and light
steps are vertex- and face-sized tensor expressions and run wherever their inputs live; rasterisation, texture sampling,
the vertical flip and the 2x2 anti-aliasing average are one call into libchore_hip.so and need device tensors.

Differentiable like the reference's: when grad mode is on and the vertices, the textures or the light require grad, the
rasterisation goes through `_RasterizeRGBAD` (chore_render_fwd + chore_render_bwd) and `render`, `render_rgb`, `render_depth`,
`render_silhouettes` and `rasterize_rgbad` carry gradients; otherwise the call is the plain forward.  The point and scene
renderers (`splat_points`, `rasterize_scene`, `render_points`, `render_scene`) are forward only and detach their inputs, and so
are visibility and instance masks (`face_visibility`, `rasterize_instances`, `Renderer.visibility`, `Renderer.render_instances`:
chore_instances_fwd; the reference's visibility.py:12-34 and renderer.py:79-117), and textures taken from a photo with the
per-texel and per-point visibility under them (`sample_depth`, `photo_textures`, `point_visibility`, `Renderer.photo_textures`,
`Renderer.vertex_visibility`: chore_photo_textures_fwd / chore_point_visibility, this package's own).

Kept quirks of the reference: `light_direction` is used un-normalised; face normals are
normalize(cross(v0 - v1, v2 - v1), eps=1e-5), dividing by max(norm, eps); lighting sees the world vertices, before the camera.
One deliberate difference: the reference multiplies the whole texture cube of every face by its light before sampling
(lighting.py:55-56); here the per-face light (B,F,3) goes to the kernel, which multiplies the blended texel -- the same
product up to fp32 rounding, without materialising lit textures.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..recon.obj_pose_roi import projection, vertices_to_faces

DEFAULT_NEAR, DEFAULT_FAR, DEFAULT_EPS = 0.1, 100.0, 1e-3      # renderer.py:16,63


def get_points_from_angles(distance, elevation, azimuth, degrees=True):
    """get_points_from_angles.py:6-24"""
    if isinstance(distance, (float, int)):
        if degrees:
            elevation, azimuth = math.radians(elevation), math.radians(azimuth)
        return (distance * math.cos(elevation) * math.sin(azimuth), distance * math.sin(elevation),
                -distance * math.cos(elevation) * math.cos(azimuth))
    if degrees:
        elevation, azimuth = math.pi / 180. * elevation, math.pi / 180. * azimuth
    return torch.stack([distance * torch.cos(elevation) * torch.sin(azimuth), distance * torch.sin(elevation),
                        -distance * torch.cos(elevation) * torch.cos(azimuth)]).transpose(1, 0)


def _vec(x, device, batch):
    t = torch.as_tensor(np.asarray(x) if isinstance(x, (list, tuple)) else x, dtype=torch.float32).to(device)
    return t[None, :].repeat(batch, 1) if t.dim() == 1 else t


def _camera(vertices, eye, target, up, target_is_point):
    """the vertices in the camera at `eye` that looks at the point `target`, or along the direction `target`"""
    if vertices.dim() != 3:
        raise ValueError("vertices Tensor should have 3 dimensions")
    B, dev = vertices.shape[0], vertices.device
    eye, target, up = _vec(eye, dev, B), _vec(target, dev, B), _vec(up, dev, B)
    z_axis = F.normalize(target - eye if target_is_point else target, eps=1e-5)
    x_axis = F.normalize(torch.cross(up, z_axis, dim=1), eps=1e-5)
    y_axis = F.normalize(torch.cross(z_axis, x_axis, dim=1), eps=1e-5)
    r = torch.stack((x_axis, y_axis, z_axis), dim=1)
    return torch.matmul(vertices - eye[:, None, :], r.transpose(1, 2))


def look_at(vertices, eye, at=(0, 0, 0), up=(0, 1, 0)):
    """look_at.py:6-62: camera at `eye` looking at `at`"""
    return _camera(vertices, eye, at, up, True)


def look(vertices, eye, direction=(0, 1, 0), up=(0, 1, 0)):
    """look.py:6-55: camera at `eye` looking along `direction` (each (3,) or (B,3); the reference's default `up` is [0, 1, 0])"""
    return _camera(vertices, eye, direction, up, False)


def perspective(vertices, angle=30.):
    """perspective.py:6-21"""
    if vertices.dim() != 3:
        raise ValueError("vertices Tensor should have 3 dimensions")
    width = torch.tan(torch.tensor(angle / 180 * math.pi, dtype=torch.float32, device=vertices.device))
    z = vertices[:, :, 2]
    return torch.stack((vertices[:, :, 0] / z / width, vertices[:, :, 1] / z / width, z), dim=2)


def face_light(faces, intensity_ambient=0.5, intensity_directional=0.5, color_ambient=(1, 1, 1),
               color_directional=(1, 1, 1), direction=(0, 1, 0)):
    """the light of lighting.py:32-52 per face: faces (B,F,3,3) world-space triangles -> (B,F,3)"""
    bs, nf = faces.shape[:2]
    dev = faces.device

    def vec(x):
        t = torch.as_tensor(np.asarray(x) if isinstance(x, (list, tuple)) else x).float().to(dev)
        return t[None, :] if t.dim() == 1 else t
    color_ambient, color_directional, direction = vec(color_ambient), vec(color_directional), vec(direction)
    light = torch.zeros(bs, nf, 3, dtype=torch.float32, device=dev)
    if intensity_ambient != 0:
        light = light + intensity_ambient * color_ambient[:, None, :]
    if intensity_directional != 0:
        f = faces.reshape(bs * nf, 3, 3)
        normals = F.normalize(torch.cross(f[:, 0] - f[:, 1], f[:, 2] - f[:, 1], dim=1), eps=1e-5).reshape(bs, nf, 3)
        cos = F.relu(torch.sum(normals * direction[:, None, :], dim=2))
        light = light + intensity_directional * (color_directional[:, None, :] * cos[:, :, None])
    return light


def lighting(faces, textures, intensity_ambient=0.5, intensity_directional=0.5, color_ambient=(1, 1, 1),
             color_directional=(1, 1, 1), direction=(0, 1, 0)):
    """lighting.py:5-57 with its signature: the lit textures (a new tensor; the reference multiplies in place).  The
    renderer does not call this -- it hands `face_light` to the kernel; kept for comparison and for callers of the reference"""
    light = face_light(faces, intensity_ambient, intensity_directional, color_ambient, color_directional, direction)
    return textures * light[:, :, None, None, None, :]


# ---- what every call into the library's rasterisers needs around it

def _ptr(x):
    return x.data_ptr() if x is not None else None


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _background(background_color):
    return (ctypes.c_float * 3)(*[float(c) for c in background_color])


def _workspace(dev, query, what, **dims):
    """the workspace of one call, query(*dims) bytes on `dev` (None: only the check); 0 bytes = a shape the library does not take"""
    if query(*dims.values()) == 0:
        raise ValueError("unsupported %s shape %s" % (what, " ".join("%s=%d" % kv for kv in dims.items())))
    return None if dev is None else torch.empty(query(*dims.values()), dtype=torch.uint8, device=dev)


def _outputs(dev, B, S, ssaa, index):
    """rgb (B,3,S,S), depth (B,S,S), alpha (B,S,S) and, if asked for, the (B,S*ssaa,S*ssaa) int32 sample index (else None)"""
    return (torch.empty(B, 3, S, S, dtype=torch.float32, device=dev), torch.empty(B, S, S, dtype=torch.float32, device=dev),
            torch.empty(B, S, S, dtype=torch.float32, device=dev),
            torch.empty(B, S * ssaa, S * ssaa, dtype=torch.int32, device=dev) if index else None)


def _opt(x, dev, shape, what, shown=None):
    """an optional tensor, detached, fp32 and contiguous on `dev`, of `shape` (named `shown` in the error); None stays None"""
    if x is None:
        return None
    x = x.detach().to(dev).float().contiguous()
    if tuple(x.shape) != shape:
        raise ValueError("%s %s expected, got %s" % (what, shown or shape, tuple(x.shape)))
    return x


def _face_group(face_group, dev, B, Fn):
    """(B,F) integer group ids as int32 on `dev`, or None"""
    if face_group is None:
        return None
    if torch.is_floating_point(face_group) or tuple(face_group.shape) != (B, Fn):
        raise ValueError("face_group: integers %s expected, got %s %s" % ((B, Fn), face_group.dtype, tuple(face_group.shape)))
    return face_group.detach().to(dev).to(torch.int32).contiguous()


def _radius(radius, dev, B, N, shown=None):
    """a number or (B,N) radii -> (the per-point radii or None, the one radius or 0.0)"""
    if torch.is_tensor(radius) and radius.dim() > 0:
        return _opt(radius, dev, (B, N), "radius: a number or", shown), 0.0
    return None, float(radius)


class _RasterizeRGBAD(torch.autograd.Function):
    """chore_render_fwd / chore_render_bwd: (tri, textures, light or None) -> rgb, depth, alpha, sample_face_index.  The
    forward is the plain call with the sample index kept; an output that receives no gradient hands NULL to the backward,
    which then leaves its term out (render_depth: no pixel-map term, render_rgb: no alpha contribution)."""

    @staticmethod
    def forward(ctx, tri, tex, light, S, ssaa, near, far, eps, background_color):
        tri, tex = tri.contiguous(), tex.contiguous()
        light = light.contiguous() if light is not None else None
        rgb, depth, alpha, fim = _render_fwd(tri, tex, light, S, ssaa, near, far, eps, background_color, True)
        ctx.save_for_backward(tri, tex, light, fim)
        ctx.args = (S, ssaa, near, far, eps, tuple(float(c) for c in background_color))
        ctx.mark_non_differentiable(fim)
        ctx.set_materialize_grads(False)          # an unused output hands None, not zeros, to the backward
        return rgb, depth, alpha, fim

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_alpha, _g_fim):
        tri, tex, light, fim = ctx.saved_tensors
        S, ssaa, near, far, eps, background = ctx.args
        dev = tri.device
        h = _lib.handle(dev.index or 0)
        B, Fn, ts = tri.shape[0], tri.shape[1], tex.shape[2]
        ws = _workspace(dev, _lib.lib.chore_render_bwd_workspace_bytes, "render", B=B, F=Fn, ts=ts, image_size=S, ssaa=ssaa)
        up = [g.float().contiguous() if g is not None else None for g in (g_rgb, g_depth, g_alpha)]
        g_tri = torch.empty_like(tri)
        g_tex = torch.empty_like(tex) if ctx.needs_input_grad[1] else None
        g_light = torch.empty_like(light) if light is not None and ctx.needs_input_grad[2] else None
        _lib.check(_lib.lib.chore_render_bwd(h, tri.data_ptr(), tex.data_ptr(), _ptr(light), fim.data_ptr(), B, Fn, ts, S, ssaa,
                                             float(near), float(far), float(eps), float(eps), _background(background),
                                             _ptr(up[0]), _ptr(up[1]), _ptr(up[2]), g_tri.data_ptr(), _ptr(g_tex), _ptr(g_light),
                                             ws.data_ptr(), _stream(dev)), h, "chore_render_bwd")
        return g_tri, g_tex, g_light, None, None, None, None, None, None


def _render_fwd(tri, tex, lt, S, ssaa, near, far, eps, background_color, return_index):
    """one chore_render_fwd call on contiguous fp32 device tensors -> rgb, depth, alpha, sample index or None"""
    dev = tri.device
    h = _lib.handle(dev.index or 0)
    B, Fn = tri.shape[:2]
    ws = _workspace(dev, _lib.lib.chore_render_workspace_bytes, "render", B=B, F=Fn, image_size=S, ssaa=ssaa)
    rgb, depth, alpha, fim = _outputs(dev, B, S, ssaa, return_index)
    _lib.check(_lib.lib.chore_render_fwd(h, tri.data_ptr(), tex.data_ptr(), _ptr(lt), B, Fn, tex.shape[2], S, ssaa, float(near),
                                         float(far), float(eps), _background(background_color), rgb.data_ptr(), depth.data_ptr(),
                                         alpha.data_ptr(), _ptr(fim), ws.data_ptr(), _stream(dev)), h, "chore_render_fwd")
    return rgb, depth, alpha, fim


def rasterize_rgbad(faces, textures, light=None, image_size=256, anti_aliasing=True, near=DEFAULT_NEAR, far=DEFAULT_FAR,
                    eps=DEFAULT_EPS, background_color=(0, 0, 0), return_index=False):
    """rasterize.py:267-348 in one call: faces (B,F,3,3) projected triangles, textures (B,F,ts,ts,ts,3), light (B,F,3) or None
    -> dict(rgb (B,3,S,S), depth (B,S,S), alpha (B,S,S)[, face_index (B,S*ssaa,S*ssaa) int32, rows not flipped]).
    Differentiable with respect to faces, textures and light when one of them requires grad and grad mode is on; `eps` is
    the reference's one eps: the clamp of the texture sampling and the distance offset of the pixel-map gradient."""
    if not faces.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    dev = faces.device
    need_grad = torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (faces, textures, light))
    keep = (lambda x: x) if need_grad else (lambda x: x.detach())
    tri = keep(faces).float().contiguous()
    tex = keep(textures).to(dev).float().contiguous()
    B, Fn = tri.shape[:2]
    ts = tex.shape[2]
    if tuple(tri.shape) != (B, Fn, 3, 3) or tuple(tex.shape) != (B, Fn, ts, ts, ts, 3):
        raise ValueError("faces (B,F,3,3) and textures (B,F,ts,ts,ts,3) expected, got %s and %s" % (tuple(tri.shape), tuple(tex.shape)))
    lt = None
    if light is not None:
        lt = keep(light).to(dev).float().contiguous()
        if tuple(lt.shape) != (B, Fn, 3):
            raise ValueError("light (B,F,3) expected")
    ssaa, S = (2 if anti_aliasing else 1), int(image_size)
    if need_grad:
        _workspace(None, _lib.lib.chore_render_workspace_bytes, "render", B=B, F=Fn, image_size=S, ssaa=ssaa)
        rgb, depth, alpha, fim = _RasterizeRGBAD.apply(tri, tex, lt, S, ssaa, near, far, eps, background_color)
    else:
        rgb, depth, alpha, fim = _render_fwd(tri, tex, lt, S, ssaa, near, far, eps, background_color, return_index)
    out = {"rgb": rgb, "depth": depth, "alpha": alpha}
    if return_index:
        out["face_index"] = fim
    return out


def splat_points(points_ndc, colors=None, radius=2.0, image_size=256, anti_aliasing=True, near=DEFAULT_NEAR, far=DEFAULT_FAR,
                 ambient=0.6, background_color=(0, 0, 0), return_index=False):
    """point clouds as shaded discs in one call (chore_splat_fwd; the rule is written down in include/chore_hip.h):
    points_ndc (B,N,3) projected points [u, v in [-1,1], depth] as `Renderer.transform` returns them, colors (B,N,3) or None =
    white, radius in output pixels: a number or (B,N)
    -> dict(rgb (B,3,S,S), depth (B,S,S), alpha (B,S,S)[, point_index (B,S*ssaa,S*ssaa) int32, rows not flipped]).
    The nearest point wins a sample, then the smallest index, whatever the order of the points.  Inputs are detached;
    N == 0 gives the background."""
    if not points_ndc.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    dev = points_ndc.device
    pts = points_ndc.detach().float().contiguous()
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise ValueError("points_ndc (B,N,3) expected, got %s" % (tuple(pts.shape),))
    B, N = pts.shape[:2]
    ssaa, S = (2 if anti_aliasing else 1), int(image_size)
    col = _opt(colors, dev, (B, N, 3), "colors", "(B,N,3)")
    rad, radius_px = _radius(radius, dev, B, N, "(B,N)")
    if N == 0:
        bgc = torch.tensor([float(c) for c in background_color], dtype=torch.float32, device=dev)
        out = {"rgb": bgc.view(1, 3, 1, 1).expand(B, 3, S, S).contiguous(),
               "depth": torch.full((B, S, S), float(far), dtype=torch.float32, device=dev),
               "alpha": torch.zeros(B, S, S, dtype=torch.float32, device=dev)}
        if return_index:
            out["point_index"] = torch.full((B, S * ssaa, S * ssaa), -1, dtype=torch.int32, device=dev)
        return out
    h = _lib.handle(dev.index or 0)
    ws = _workspace(dev, _lib.lib.chore_splat_workspace_bytes, "splat", B=B, N=N, image_size=S, ssaa=ssaa)
    rgb, depth, alpha, pim = _outputs(dev, B, S, ssaa, return_index)
    _lib.check(_lib.lib.chore_splat_fwd(h, pts.data_ptr(), _ptr(col), _ptr(rad), radius_px, B, N, S, ssaa, float(ambient),
                                        float(near), float(far), _background(background_color), rgb.data_ptr(), depth.data_ptr(),
                                        alpha.data_ptr(), _ptr(pim), ws.data_ptr(), _stream(dev)), h, "chore_splat_fwd")
    out = {"rgb": rgb, "depth": depth, "alpha": alpha}
    if return_index:
        out["point_index"] = pim
    return out


def rasterize_scene(faces, textures, light, points_ndc, colors=None, radius=2.0, face_opacity=None, point_depth_bias=0.0,
                    image_size=256, anti_aliasing=True, near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=DEFAULT_EPS, ambient=0.6,
                    background_color=(0, 0, 0), return_index=False, face_layers=1, face_group=None):
    """meshes and point clouds in ONE image, depth-tested against each other per sample before the anti-aliasing average
    (chore_scene_fwd; the rule is written down in include/chore_hip.h).  faces / textures / light as `rasterize_rgbad` takes
    them, points_ndc / colors / radius as `splat_points` does; face_opacity (B,F) in [0,1] or None = opaque; point_depth_bias
    >= 0 (depth units) lets a point that lies ON a surface win against it.
    face_layers (1..8): how many faces a sample composites front to back.  With the default 1 a translucent face shows the
    nearest point behind it or the background, never another face; with more (chore_scene_layers_fwd) it shows the faces
    behind it too, down to the first opaque one or the point.  face_group (B,F) integers or None: of the faces with one group id
    only the nearest counts, so a translucent closed mesh given as one group adds one layer and not also its own back side.
    -> dict(rgb (B,3,S,S), depth (B,S,S), alpha (B,S,S)[, sample_id (B,S*ssaa,S*ssaa) int32, rows not flipped: f >= 0 a face,
    -2 - n a point, -1 nothing]).  F == 0 is `splat_points`; N == 0 is `rasterize_rgbad` when every face is opaque, and the
    scene kernel with one point that is never drawn when there is a face_opacity to honour."""
    if not faces.is_cuda or not points_ndc.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    bias = float(point_depth_bias)
    if not bias >= 0.0:
        raise ValueError("point_depth_bias must be >= 0, got %r" % (point_depth_bias,))
    layers = int(face_layers)
    if not 1 <= layers <= 8:
        raise ValueError("face_layers must lie in 1..8, got %r" % (face_layers,))
    dev = faces.device
    tri = faces.detach().float().contiguous()
    pts = points_ndc.detach().to(dev).float().contiguous()
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise ValueError("points_ndc (B,N,3) expected, got %s" % (tuple(pts.shape),))
    if tri.dim() != 4 or pts.shape[0] != tri.shape[0]:
        raise ValueError("faces (B,F,3,3) and points_ndc (B,N,3) of one batch size expected, got %s and %s"
                         % (tuple(tri.shape), tuple(pts.shape)))
    B, Fn, N = tri.shape[0], tri.shape[1], pts.shape[1]
    grp = _face_group(face_group, dev, B, Fn)
    if Fn == 0:
        out = splat_points(pts, colors, radius, image_size, anti_aliasing, near, far, ambient, background_color, return_index)
        if return_index:
            pim = out.pop("point_index")
            out["sample_id"] = torch.where(pim >= 0, -2 - pim, pim)
        return out
    if N == 0 and face_opacity is not None:        # z == far is skipped by the point rule
        pts, colors, radius, N = torch.tensor([0.0, 0.0, float(far)], device=dev).expand(B, 1, 3).contiguous(), None, 1.0, 1
    if N == 0:
        out = rasterize_rgbad(tri, textures.detach(), None if light is None else light.detach(), image_size, anti_aliasing,
                              near, far, eps, background_color, return_index)
        if return_index:
            out["sample_id"] = out.pop("face_index")
        return out
    tex = textures.detach().to(dev).float().contiguous()
    ts = tex.shape[2]
    if tuple(tri.shape) != (B, Fn, 3, 3) or tuple(tex.shape) != (B, Fn, ts, ts, ts, 3):
        raise ValueError("faces (B,F,3,3) and textures (B,F,ts,ts,ts,3) expected, got %s and %s" % (tuple(tri.shape), tuple(tex.shape)))
    lt, col = _opt(light, dev, (B, Fn, 3), "light"), _opt(colors, dev, (B, N, 3), "colors")
    op = _opt(face_opacity, dev, (B, Fn), "face_opacity")
    rad, radius_px = _radius(radius, dev, B, N)
    ssaa, S = (2 if anti_aliasing else 1), int(image_size)
    h = _lib.handle(dev.index or 0)
    ws = _workspace(dev, _lib.lib.chore_scene_workspace_bytes, "scene", B=B, F=Fn, N=N, image_size=S, ssaa=ssaa)
    rgb, depth, alpha, sid = _outputs(dev, B, S, ssaa, return_index)
    head = (h, tri.data_ptr(), tex.data_ptr(), _ptr(lt), _ptr(op), B, Fn, ts, pts.data_ptr(), _ptr(col), _ptr(rad), radius_px, N, bias,
            S, ssaa, float(ambient), float(near), float(far), float(eps), _background(background_color))
    tail = (rgb.data_ptr(), depth.data_ptr(), alpha.data_ptr(), _ptr(sid), ws.data_ptr(), _stream(dev))
    if layers == 1 and grp is None:
        _lib.check(_lib.lib.chore_scene_fwd(*head, *tail), h, "chore_scene_fwd")
    else:
        _lib.check(_lib.lib.chore_scene_layers_fwd(*head, _ptr(grp), layers, *tail), h, "chore_scene_layers_fwd")
    out = {"rgb": rgb, "depth": depth, "alpha": alpha}
    if return_index:
        out["sample_id"] = sid
    return out


MAX_GROUPS = 8        # chore_instances_fwd keeps an 8-bit cover mask per sample


def rasterize_instances(faces, face_group=None, num_groups=1, image_size=256, anti_aliasing=True, near=DEFAULT_NEAR,
                        far=DEFAULT_FAR, return_index=False):
    """which group of faces owns a pixel, and which groups would cover it alone, in one walk (chore_instances_fwd; the rule is
    written down in include/chore_hip.h).  faces (B,F,3,3) projected triangles as `rasterize_rgbad` takes them; face_group
    (B,F) integers or None = every face in group 0; num_groups G in 1..8.  A face whose group lies outside 0..G-1 is an
    occluder: it hides what is behind it and belongs to no group.
    -> dict(visible (B,G,S,S): coverage of the group as seen; full (B,G,S,S): its coverage with every other face taken away;
    face_samples (B,F) int32: samples each face wins; group_samples (B,G,2) int32: samples of visible / full
    [, face_index (B,S*ssaa,S*ssaa) int32, rows not flipped]).  Forward only: the inputs are detached."""
    if not faces.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    G = int(num_groups)
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError("num_groups must lie in 1..%d, got %r" % (MAX_GROUPS, num_groups))
    dev = faces.device
    tri = faces.detach().float().contiguous()
    if tri.dim() != 4 or tuple(tri.shape[2:]) != (3, 3):
        raise ValueError("faces (B,F,3,3) expected, got %s" % (tuple(tri.shape),))
    B, Fn = tri.shape[:2]
    grp = _face_group(face_group, dev, B, Fn)
    ssaa, S = (2 if anti_aliasing else 1), int(image_size)
    h = _lib.handle(dev.index or 0)
    ws = _workspace(dev, _lib.lib.chore_instances_workspace_bytes, "instances", B=B, F=Fn, G=G, image_size=S, ssaa=ssaa)
    visible = torch.empty(B, G, S, S, dtype=torch.float32, device=dev)
    full = torch.empty(B, G, S, S, dtype=torch.float32, device=dev)
    face_samples = torch.empty(B, Fn, dtype=torch.int32, device=dev)
    group_samples = torch.empty(B, G, 2, dtype=torch.int32, device=dev)
    fim = torch.empty(B, S * ssaa, S * ssaa, dtype=torch.int32, device=dev) if return_index else None
    _lib.check(_lib.lib.chore_instances_fwd(h, tri.data_ptr(), _ptr(grp), B, Fn, G, S, ssaa, float(near), float(far),
                                            visible.data_ptr(), full.data_ptr(), face_samples.data_ptr(), group_samples.data_ptr(),
                                            _ptr(fim), ws.data_ptr(), _stream(dev)), h, "chore_instances_fwd")
    out = {"visible": visible, "full": full, "face_samples": face_samples, "group_samples": group_samples}
    if return_index:
        out["face_index"] = fim
    return out


def face_visibility(faces, image_size, near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=1e-4):
    """visibility.py:12-34 with its signature: faces (B,F,3,3) projected triangles -> (B,F) int32, 1 where the face wins at
    least one pixel of the image_size grid (no anti-aliasing).  `eps` is accepted and not read, as in the reference."""
    if not faces.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    out = rasterize_instances(faces, None, 1, image_size, False, near, far)
    return (out["face_samples"] > 0).to(torch.int32)


VISIBILITY_DEPTH_BIAS = 0.02      # depth units of the triangles (metres in camera views): the fitter's VIEW_POINT_BIAS, not tuned


def _projected_faces(faces):
    if not faces.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    tri = faces.detach().float().contiguous()
    if tri.dim() != 4 or tuple(tri.shape[2:]) != (3, 3) or tri.shape[0] < 1 or tri.shape[1] < 1:
        raise ValueError("faces (B,F,3,3) expected, got %s" % (tuple(tri.shape),))
    return tri


def _depth_image(depth, dev, B):
    d = depth.detach().to(dev).float().contiguous()
    if d.dim() != 3 or d.shape[0] != B or d.shape[1] != d.shape[2]:
        raise ValueError("depth (B,S,S) with B = %d expected, got %s" % (B, tuple(d.shape)))
    if not 1 <= d.shape[1] <= 4096:
        raise ValueError("depth: S must lie in 1..4096, got %d" % d.shape[1])
    return d


def sample_depth(faces, image_size, near=DEFAULT_NEAR, far=DEFAULT_FAR):
    """faces (B,F,3,3) projected triangles -> (B,S,S) depth of the nearest face per sample of the image_size grid without
    anti-aliasing, rows NOT flipped, `far` where there is none: the depth image `photo_textures` and `point_visibility` test
    against (chore_silhouette_fwd + chore_sil_depth; `rasterize_rgbad`'s depth at anti_aliasing=False with the rows reversed).
    Forward only: the input is detached."""
    tri = _projected_faces(faces)
    dev, S = tri.device, int(image_size)
    if not 1 <= S <= 4096:
        raise ValueError("image_size must lie in 1..4096, got %r" % (image_size,))
    B, Fn = tri.shape[:2]
    h = _lib.handle(dev.index or 0)
    fim = torch.empty(B, S, S, dtype=torch.int32, device=dev)
    alpha = torch.empty(B, S, S, dtype=torch.float32, device=dev)
    depth = torch.empty(B, S, S, dtype=torch.float32, device=dev)
    ws = torch.empty(max(_lib.lib.chore_silhouette_workspace_bytes(B, Fn), 1), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.chore_silhouette_fwd(h, tri.data_ptr(), B, Fn, S, float(near), float(far), fim.data_ptr(), alpha.data_ptr(),
                                             ws.data_ptr(), _stream(dev)), h, "chore_silhouette_fwd")
    _lib.check(_lib.lib.chore_sil_depth(h, tri.data_ptr(), fim.data_ptr(), B, Fn, S, float(far), 0, depth.data_ptr(), _stream(dev)),
               h, "chore_sil_depth")
    return depth


def photo_textures(faces, depth, photo, fallback, texture_size=4, depth_bias=VISIBILITY_DEPTH_BIAS, near=DEFAULT_NEAR,
                   far=DEFAULT_FAR, align_corners=False, return_visible=False):
    """the texture cube of every face filled from a photo at the texels the camera sees (chore_photo_textures_fwd; the rule is
    written down in include/chore_hip.h).  faces (B,F,3,3) projected triangles as `rasterize_rgbad` takes them; depth (B,S,S)
    from `sample_depth` (of these faces or of a larger scene that hides them); photo (B,3,Hp,Wp) in the orientation of an
    image (row 0 on top): Wp is the side of the square [-1,1]^2 maps to, of which the upper Hp <= Wp rows exist; fallback
    (B,F,3): the colour of a texel that is hidden, out of view or outside the photo.  depth_bias is in the depth units of the
    triangles (metres in camera views); 0.02 is the fitter's VIEW_POINT_BIAS, not tuned.  align_corners=True reads the photo
    under grid_sample's align_corners=True convention, which KinectColorCamera.project_points produces.
    -> textures (B,F,ts,ts,ts,3) [, visible (B,F,ts,ts,ts) bool].  Forward only: the inputs are detached."""
    tri = _projected_faces(faces)
    dev = tri.device
    B, Fn = tri.shape[:2]
    ts = int(texture_size)
    if not 2 <= ts <= 16:
        raise ValueError("texture_size must lie in 2..16, got %r" % (texture_size,))
    d = _depth_image(depth, dev, B)
    ph = photo.detach().to(dev).float().contiguous()
    if ph.dim() != 4 or ph.shape[0] != B or ph.shape[1] != 3 or ph.shape[2] < 1 or ph.shape[2] > ph.shape[3]:
        raise ValueError("photo (B,3,Hp,Wp) with B = %d and 1 <= Hp <= Wp expected, got %s" % (B, tuple(ph.shape)))
    fb = _opt(fallback, dev, (B, Fn, 3), "fallback")
    if fb is None:
        raise ValueError("fallback (B,F,3) expected")
    tex = torch.empty(B, Fn, ts, ts, ts, 3, dtype=torch.float32, device=dev)
    vis = torch.empty(B, Fn, ts, ts, ts, dtype=torch.uint8, device=dev) if return_visible else None
    h = _lib.handle(dev.index or 0)
    _lib.check(_lib.lib.chore_photo_textures_fwd(h, tri.data_ptr(), d.data_ptr(), ph.data_ptr(), fb.data_ptr(), B, Fn, ts,
                                                 d.shape[1], ph.shape[2], ph.shape[3], float(near), float(far), float(depth_bias),
                                                 1 if align_corners else 0, tex.data_ptr(), _ptr(vis), _stream(dev)),
               h, "chore_photo_textures_fwd")
    return (tex, vis.bool()) if return_visible else tex


def point_visibility(points, depth, depth_bias=VISIBILITY_DEPTH_BIAS, near=DEFAULT_NEAR, far=DEFAULT_FAR):
    """projected points (B,N,3) [u, v in [-1,1], depth] against a depth image (B,S,S) from `sample_depth` -> (B,N) int32, 1 where
    the point is in view, between near and far, and not more than depth_bias behind the nearest face of its sample
    (chore_point_visibility: the rule `photo_textures` applies to a texel).  depth_bias as in `photo_textures`.  Forward only."""
    if not points.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    pts = points.detach().float().contiguous()
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[0] < 1 or pts.shape[1] < 1:
        raise ValueError("points (B,N,3) expected, got %s" % (tuple(pts.shape),))
    dev = pts.device
    B, N = pts.shape[:2]
    d = _depth_image(depth, dev, B)
    out = torch.empty(B, N, dtype=torch.int32, device=dev)
    h = _lib.handle(dev.index or 0)
    _lib.check(_lib.lib.chore_point_visibility(h, pts.data_ptr(), d.data_ptr(), B, N, d.shape[1], float(near), float(far),
                                               float(depth_bias), out.data_ptr(), _stream(dev)), h, "chore_point_visibility")
    return out


def world_radius_to_pixels(world_radius, z, focal_px):
    """pixel radius of a sphere of `world_radius` metres at depth z under a focal length of `focal_px` OUTPUT pixels:
    focal_px * world_radius / z, so points shrink with distance"""
    return focal_px * world_radius / z


class Renderer(nn.Module):
    """neural_renderer.Renderer (renderer.py:11-63): same constructor arguments and attributes.  K / R / t may live on any
    device; they are moved to the vertices' device when rendering."""

    def __init__(self, image_size=256, anti_aliasing=True, background_color=[0, 0, 0], fill_back=True,
                 camera_mode="projection", K=None, R=None, t=None, dist_coeffs=None, orig_size=1024, perspective=True,
                 viewing_angle=30, camera_direction=[0, 0, 1], near=0.1, far=100, light_intensity_ambient=0.5,
                 light_intensity_directional=0.5, light_color_ambient=[1, 1, 1], light_color_directional=[1, 1, 1],
                 light_direction=[0, 1, 0]):
        super().__init__()
        self.image_size = image_size
        self.anti_aliasing = anti_aliasing
        self.background_color = background_color
        self.fill_back = fill_back
        self.camera_mode = camera_mode
        if camera_mode == "projection":
            as_t = lambda x: torch.as_tensor(x, dtype=torch.float32) if isinstance(x, np.ndarray) else x    # noqa: E731
            self.K, self.R, self.t = as_t(K), as_t(R), as_t(t)
            self.dist_coeffs = torch.zeros(1, 5) if dist_coeffs is None else dist_coeffs
            self.orig_size = orig_size
        elif camera_mode in ("look", "look_at"):
            self.perspective = perspective
            self.viewing_angle = viewing_angle
            self.eye = [0, 0, -(1. / math.tan(math.radians(self.viewing_angle)) + 1)]
            self.camera_direction = [0, 0, 1]
        else:
            raise ValueError("Camera mode has to be one of projection, look or look_at")
        self.near = near
        self.far = far
        self.light_intensity_ambient = light_intensity_ambient
        self.light_intensity_directional = light_intensity_directional
        self.light_color_ambient = light_color_ambient
        self.light_color_directional = light_color_directional
        self.light_direction = light_direction
        self.rasterizer_eps = 1e-3

    def forward(self, vertices, faces, textures=None, mode=None, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        if mode is None:
            return self.render(vertices, faces, textures, K, R, t, dist_coeffs, orig_size)
        if mode == "rgb":
            return self.render_rgb(vertices, faces, textures, K, R, t, dist_coeffs, orig_size)
        if mode == "silhouettes":
            return self.render_silhouettes(vertices, faces, K, R, t, dist_coeffs, orig_size)
        if mode == "depth":
            return self.render_depth(vertices, faces, K, R, t, dist_coeffs, orig_size)
        if mode == "visibility":
            return self.visibility(vertices, faces, K, R, t, dist_coeffs, orig_size)
        raise ValueError("mode should be one of None, 'rgb', 'silhouettes', 'depth' or 'visibility'")

    def transform(self, vertices, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """world vertices (B,V,3) -> [u, v in [-1,1], depth] under the camera mode (renderer.py:254-276)"""
        if self.camera_mode == "look_at":
            vertices = look_at(vertices, self.eye)
            return perspective(vertices, angle=self.viewing_angle) if self.perspective else vertices
        if self.camera_mode == "look":
            raise NotImplementedError("camera mode 'look' is not provided")
        dev = vertices.device
        K = self.K if K is None else K
        R = self.R if R is None else R
        t = self.t if t is None else t
        dist_coeffs = self.dist_coeffs if dist_coeffs is None else dist_coeffs
        orig_size = self.orig_size if orig_size is None else orig_size
        on = lambda x: torch.as_tensor(x, dtype=torch.float32).to(dev)     # noqa: E731
        return projection(vertices, on(K), on(R), on(t), on(dist_coeffs), orig_size)

    def _prepare_faces(self, vertices, faces, textures, cam, face_opacity=None, projected=None):
        """what the rasteriser needs of a mesh: projected triangles, textures, light (None without textures), opacity -- with
        both windings when fill_back is set (renderer.py:119-152).  projected (B,V,3): the vertices under a camera of the
        caller's instead of this renderer's (the light always sees the world vertices)"""
        vertices = vertices.float()           # attached: the light and the camera are torch expressions of the vertices
        faces = faces.detach()
        light = None
        if textures is None:        # coverage / depth only: one white texel cube per face
            textures = torch.ones(faces.shape[0], faces.shape[1], 2, 2, 2, 3, dtype=torch.float32, device=vertices.device)
            lit = False
        else:
            textures = textures.to(vertices.device).float()
            lit = True
        if self.fill_back:
            faces = torch.cat((faces, faces.flip(-1)), dim=1)
            textures = torch.cat((textures, textures.permute((0, 1, 4, 3, 2, 5))), dim=1)
            if face_opacity is not None:
                face_opacity = torch.cat((face_opacity, face_opacity), dim=1)
        if lit:
            light = face_light(vertices_to_faces(vertices, faces), self.light_intensity_ambient,
                               self.light_intensity_directional, self.light_color_ambient, self.light_color_directional,
                               self.light_direction)
        tri = vertices_to_faces(self.transform(vertices, *cam) if projected is None else projected, faces)
        return tri, textures, light, face_opacity

    def _rasterize(self, vertices, faces, textures, cam, return_index=False):
        tri, textures, light, _ = self._prepare_faces(vertices, faces, textures, cam)
        return rasterize_rgbad(tri, textures, light, self.image_size, self.anti_aliasing, self.near, self.far,
                               self.rasterizer_eps, self.background_color, return_index=return_index)

    def render(self, vertices, faces, textures, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """-> (rgb (B,3,S,S), depth (B,S,S), alpha (B,S,S))   (renderer.py:237-283); differentiable with respect to the
        vertices and the textures"""
        out = self._rasterize(vertices, faces, textures, (K, R, t, dist_coeffs, orig_size))
        return out["rgb"], out["depth"], out["alpha"]

    def render_rgb(self, vertices, faces, textures, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        return self._rasterize(vertices, faces, textures, (K, R, t, dist_coeffs, orig_size))["rgb"]

    def render_depth(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        return self._rasterize(vertices, faces, None, (K, R, t, dist_coeffs, orig_size))["depth"]

    def render_silhouettes(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        return self._rasterize(vertices, faces, None, (K, R, t, dist_coeffs, orig_size))["alpha"]

    def _project_faces(self, vertices, faces, cam, face_group=None):
        """projected triangles of a mesh, detached, with both windings (and their groups) when fill_back is set"""
        faces = faces.detach()
        if self.fill_back:
            faces = torch.cat((faces, faces.flip(-1)), dim=1)
            if face_group is not None:
                face_group = torch.cat((face_group, face_group), dim=1)
        return vertices_to_faces(self.transform(vertices.detach().float(), *cam), faces), face_group

    def visibility(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """-> (B,F) int32, (B,2F) with fill_back: 1 where the face wins a pixel (renderer.py:84-117).  Like the reference it
        rasterises at image_size without anti-aliasing, whatever self.anti_aliasing says.  Forward only."""
        tri, _ = self._project_faces(vertices, faces, (K, R, t, dist_coeffs, orig_size))
        return face_visibility(tri, self.image_size, near=self.near, far=self.far)

    def render_instances(self, vertices, faces, face_group=None, num_groups=1, K=None, R=None, t=None, dist_coeffs=None,
                         orig_size=None):
        """the camera path of `render`, then `rasterize_instances`: face_group (B,F) integers per face of `faces` (both windings
        get them under fill_back) or None -> its dict (face_samples is (B,2F) under fill_back).  Forward only."""
        if face_group is not None:
            face_group = torch.as_tensor(face_group).to(vertices.device)
        tri, face_group = self._project_faces(vertices, faces, (K, R, t, dist_coeffs, orig_size), face_group)
        return rasterize_instances(tri, face_group, num_groups, self.image_size, self.anti_aliasing, self.near, self.far)

    def _visibility_depth(self, vertices, faces, visibility_size, cam):
        """projected vertices (B,V,3), detached, and the depth image of the mesh (both windings under fill_back) at
        visibility_size (None: image_size), without anti-aliasing"""
        ndc = self.transform(vertices.detach().float(), *cam)
        faces = faces.detach()
        both = torch.cat((faces, faces.flip(-1)), dim=1) if self.fill_back else faces
        S = self.image_size if visibility_size is None else visibility_size
        return ndc, sample_depth(vertices_to_faces(ndc, both), S, self.near, self.far)

    def photo_textures(self, vertices, faces, photo, fallback=None, texture_size=4, depth_bias=VISIBILITY_DEPTH_BIAS,
                       visibility_size=None, K=None, R=None, t=None, dist_coeffs=None, orig_size=None, align_corners=False,
                       return_visible=False):
        """the camera path of `render`, then `photo_textures`: textures (B,F,ts,ts,ts,3) for the F faces given, coloured from
        `photo` (B,3,Hp,Wp) where this camera sees them, so `render(vertices, faces, textures)` doubles them under fill_back as
        it does any textures.  The depth image is taken over both windings under fill_back, at visibility_size (None:
        image_size) without anti-aliasing.  fallback: one colour (3,), (B,F,3), or None = mid grey.  depth_bias: depth units of
        the camera (metres in camera views); 0.02 is the fitter's VIEW_POINT_BIAS, not tuned.  Forward only."""
        ndc, depth = self._visibility_depth(vertices, faces, visibility_size, (K, R, t, dist_coeffs, orig_size))
        B, Fn = faces.shape[:2]
        fb = torch.as_tensor((0.5, 0.5, 0.5) if fallback is None else fallback, dtype=torch.float32).to(ndc.device)
        if fb.dim() == 1:
            fb = fb.view(1, 1, 3).expand(B, Fn, 3)
        return photo_textures(vertices_to_faces(ndc, faces.detach()), depth, photo, fb, texture_size, depth_bias, self.near,
                              self.far, align_corners, return_visible)

    def vertex_visibility(self, vertices, faces, depth_bias=VISIBILITY_DEPTH_BIAS, visibility_size=None, K=None, R=None, t=None,
                          dist_coeffs=None, orig_size=None):
        """-> (B,V) int32: 1 where the vertex is in view and not more than depth_bias behind the nearest face of its sample
        (`point_visibility` against the mesh's own depth image, both windings under fill_back).  Forward only."""
        ndc, depth = self._visibility_depth(vertices, faces, visibility_size, (K, R, t, dist_coeffs, orig_size))
        return point_visibility(ndc, depth, depth_bias, self.near, self.far)

    def focal_pixels(self, K=None, orig_size=None):
        """focal length in pixels of THIS renderer's output: K[0,0] scaled from `orig_size` to image_size in projection
        mode ((B,) tensor or a number), (image_size / 2) / tan(viewing_angle) in look_at mode (perspective() divides by
        tan(angle) and the normalised half-width 1 is image_size / 2 pixels)"""
        if self.camera_mode == "projection":
            K = self.K if K is None else K
            orig_size = self.orig_size if orig_size is None else orig_size
            fx = torch.as_tensor(K, dtype=torch.float32).reshape(-1, 3, 3)[:, 0, 0]
            return fx * (self.image_size / float(orig_size))
        return 0.5 * self.image_size / math.tan(math.radians(self.viewing_angle))

    def render_points(self, points, colors=None, radius=2.0, world_radius=None, K=None, R=None, t=None, dist_coeffs=None,
                      orig_size=None):
        """world points (B,N,3) as shaded discs -> (rgb (B,3,S,S), depth (B,S,S), alpha (B,S,S)); inputs are detached.
        radius: output pixels, a number or (B,N).  world_radius (metres, a number or (B,N)) replaces it by the per-point
        pixel radius focal_px * world_radius / z."""
        ndc, radius = self._prepare_points(points, radius, world_radius, (K, R, t, dist_coeffs, orig_size))
        out = splat_points(ndc, colors, radius, self.image_size, self.anti_aliasing, self.near, self.far,
                           background_color=self.background_color)
        return out["rgb"], out["depth"], out["alpha"]

    def _prepare_points(self, points, radius, world_radius, cam):
        """projected points and their radius in output pixels (`radius`, or focal_px * world_radius / z)"""
        K, orig_size = cam[0], cam[4]
        ndc = self.transform(points.detach().float(), *cam)
        if world_radius is not None:
            focal = self.focal_pixels(K, orig_size)
            if torch.is_tensor(focal):
                focal = focal.to(ndc.device).view(-1, 1)
            wr = torch.as_tensor(world_radius, dtype=torch.float32).to(ndc.device)
            radius = world_radius_to_pixels(wr, ndc[:, :, 2], focal).expand(ndc.shape[0], ndc.shape[1])
        return ndc, radius

    def render_scene(self, vertices, faces, textures, points, colors=None, radius=2.0, world_radius=None, face_opacity=None,
                     point_depth_bias=0.0, K=None, R=None, t=None, dist_coeffs=None, orig_size=None, face_layers=1,
                     face_group=None):
        """a mesh (as `render` takes it) and world points (as `render_points` takes them) in one image, occluding each other
        per sample -> (rgb (B,3,S,S), depth (B,S,S), alpha (B,S,S)); inputs are detached.  face_opacity (B,F) or None =
        opaque, and face_group (B,F) integers or None, per face of `faces` (both windings get them under fill_back);
        point_depth_bias, face_layers, face_group: see `rasterize_scene`."""
        cam = (K, R, t, dist_coeffs, orig_size)
        if face_group is not None:
            face_group = torch.as_tensor(face_group).to(vertices.device)
            if self.fill_back:
                face_group = torch.cat((face_group, face_group), dim=1)
        if face_opacity is not None:
            face_opacity = torch.as_tensor(face_opacity, dtype=torch.float32).to(vertices.device)
        tri, textures, light, face_opacity = self._prepare_faces(vertices, faces, textures, cam, face_opacity)
        ndc, radius = self._prepare_points(points.to(vertices.device), radius, world_radius, cam)
        out = rasterize_scene(tri, textures, light, ndc, colors, radius, face_opacity, point_depth_bias, self.image_size,
                              self.anti_aliasing, self.near, self.far, self.rasterizer_eps,
                              background_color=self.background_color, face_layers=face_layers, face_group=face_group)
        return out["rgb"], out["depth"], out["alpha"]
