"""Generate tests/golden/render_host.npz by running THE REFERENCE's own host-side rendering code on CPU tensors.

Run in the build container only (needs /root/reference):

    python tests/golden/make_render_golden.py

neural_renderer's package __init__ pulls in its CUDA extension and cannot be imported, so lighting.py, look_at.py,
perspective.py, get_points_from_angles.py, projection.py and vertices_to_faces.py are loaded by path under a stand-in
`neural_renderer` package.  utils/render_utils.py imports cv2, psbody.mesh and neural_renderer at module level; stand-ins
are put into sys.modules for the import (the same mechanism make_golden.py uses for the fit drivers).  The cv2 stand-in
provides a `resize` that asserts equal sizes and returns its input: align_to_input is recorded only on cases where
crop_size == train_crop_size, where cv2.resize is the identity, i.e. its crop / pad / index arithmetic.

The fixture holds arrays only: seeded inputs, the reference's float32 results, and for every float32 result `bound_<name>`,
the largest difference between it and the same formula evaluated in float64 by this script (the tests allow 4 x that).
"""
import importlib.util
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
NR_DIR = os.path.join(REF, "external", "neural_renderer", "neural_renderer")


class _Mesh:
    def __init__(self, v=None, f=None):
        if v is not None:
            self.v = np.array(v, dtype=np.float64)
        if f is not None:
            self.f = np.array(f)


def load_reference():
    pkg = types.ModuleType("neural_renderer")
    pkg.__path__ = [NR_DIR]
    sys.modules["neural_renderer"] = pkg
    for name in ("lighting", "look_at", "perspective", "get_points_from_angles", "projection", "vertices_to_faces"):
        spec = importlib.util.spec_from_file_location("neural_renderer." + name, os.path.join(NR_DIR, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        setattr(pkg, name, getattr(mod, name))
    rmod = types.ModuleType("neural_renderer.renderer")
    rmod.Renderer = pkg.Renderer = object
    sys.modules["neural_renderer.renderer"] = rmod
    cv2 = types.ModuleType("cv2")

    def resize(img, dsize):
        assert (img.shape[1], img.shape[0]) == tuple(dsize), "recorded only where cv2.resize is the identity"
        return img
    cv2.resize = resize
    sys.modules["cv2"] = cv2
    ps, psm = types.ModuleType("psbody"), types.ModuleType("psbody.mesh")
    psm.Mesh = _Mesh
    ps.mesh = psm
    sys.modules["psbody"], sys.modules["psbody.mesh"] = ps, psm
    sys.path.insert(0, REF)
    import utils.render_utils as ru
    return pkg, ru


def pattern(h, w):
    """the rendering stand-in of the align_to_input cases (the test rebuilds it from this formula)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 3 + yy * 5) % 251, (xx * 7 + yy * 2) % 241, (xx + yy * 11) % 239], -1).astype(np.uint8)


def light64(tri, ia, idir, direction):
    t = tri.astype(np.float64)
    n = np.cross(t[:, :, 0] - t[:, :, 1], t[:, :, 2] - t[:, :, 1])
    n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-5)
    cos = np.maximum((n * np.asarray(direction, np.float64)).sum(-1), 0.0)
    return (ia + idir * cos)[..., None] * np.ones(3)


def main():
    nr, ru = load_reference()
    rs = np.random.RandomState(2024)
    out = {}
    # two seeded meshes around the camera axis at 2.2 m
    meshes = []
    for nv, nf, c, s in ((60, 100, (-0.1, 0.05, 2.2), 0.45), (50, 80, (0.5, -0.1, 2.4), 0.25)):
        v = rs.standard_normal((nv, 3)) * s + np.asarray(c)
        f = np.stack([rs.choice(nv, 3, replace=False) for _ in range(nf)]).astype(np.int64)
        meshes.append(_Mesh(v=v, f=f))
    for i, m in enumerate(meshes):
        out["mesh%d_v" % i], out["mesh%d_f" % i] = m.v, m.f
    wrap = ru.NrWrapper.__new__(ru.NrWrapper)
    wrap.device, wrap.colors = "cpu", [list(c) for c in ru.SMPL_OBJ_COLOR_LIST]
    verts, faces, textures = wrap.prepare_render(meshes)
    out["comb_verts"], out["comb_faces"], out["comb_textures"] = verts.numpy(), faces.numpy(), textures.numpy()
    out["colors"] = np.asarray(ru.SMPL_OBJ_COLOR_LIST, np.float64)

    # lighting on the doubled list (renderer.py:239-252), random textures of size 2
    faces2 = torch.cat((faces, faces.flip(-1)), dim=1)
    tex = torch.from_numpy(rs.uniform(0, 1, (1, faces.shape[1], 2, 2, 2, 3)).astype(np.float32))
    tex2 = torch.cat((tex, tex.permute((0, 1, 4, 3, 2, 5))), dim=1)
    out["light_textures"] = tex.numpy()
    eye = nr.get_points_from_angles(2.0, 0., 90.)
    out["side_eye"] = np.asarray(eye, np.float64)
    settings = {"front": (0.4, 0.3, [1, 0.5, 1]), "side": (0.5, 0.3, list(np.array(eye) / 2.2))}
    tri_world = nr.vertices_to_faces(verts, faces2)
    out["tri_world"] = tri_world.numpy()
    for name, (ia, idir, direction) in settings.items():
        lit = nr.lighting(tri_world, tex2.clone(), ia, idir, [1, 1, 1], [1, 1, 1], direction).numpy()
        l64 = light64(tri_world.numpy(), ia, idir, direction)
        want = tex2.numpy().astype(np.float64) * l64[:, :, None, None, None, :]
        out["lit_" + name] = lit
        out["light64_" + name] = l64
        out["light_args_" + name] = np.asarray([ia, idir] + list(direction), np.float64)
        out["bound_lit_" + name] = np.abs(lit - want).max()

    # projection under the Kinect intrinsics of get_kinect_K(2048) (the function itself builds CUDA tensors)
    K = np.array([[[979.784, 0, 1018.952], [0, 979.840, 779.486], [0, 0, 1]]], np.float32)
    R, t, dist = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32), np.zeros((1, 5), np.float32)
    proj = nr.projection(verts, torch.from_numpy(K), torch.from_numpy(R), torch.from_numpy(t), torch.from_numpy(dist), 2048.0).numpy()
    v64 = verts.numpy().astype(np.float64)
    x_, y_ = v64[..., 0] / (v64[..., 2] + 1e-9), v64[..., 1] / (v64[..., 2] + 1e-9)
    K64 = K.astype(np.float64)[0]
    u = K64[0, 0] * x_ + K64[0, 2]
    vv = 2048.0 - (K64[1, 1] * y_ + K64[1, 2])
    p64 = np.stack([2 * (u - 1024.0) / 2048.0, 2 * (vv - 1024.0) / 2048.0, v64[..., 2]], -1)
    out["kinect_K"], out["proj"], out["bound_proj"] = K, proj, np.abs(proj - p64).max()

    # the side view: rotate, normalise, centre (prepare_side_rend), look_at + perspective
    rot = wrap.rotate_meshes(meshes)
    out["norm_scale"] = np.float64(ru.cal_norm_scale(rot, 1.8))
    sfaces, stexts, sverts = wrap.prepare_side_rend(meshes, maxd=1.8)
    out["side_verts"] = sverts.numpy()
    assert np.array_equal(sfaces.numpy(), faces.numpy()) and np.array_equal(stexts.numpy(), textures.numpy())
    r64 = np.concatenate([m.v * [1, -1, 1] for m in meshes]) * out["norm_scale"]
    r64 = r64.astype(np.float32).astype(np.float64)          # prepare_render rounds the vertices to float32
    r64 = r64 - r64.mean(0)
    out["bound_side_verts"] = np.abs(sverts.numpy()[0] - r64).max()
    cam = nr.perspective(nr.look_at(sverts, eye), angle=30.).numpy()
    s64 = sverts.numpy().astype(np.float64)[0]
    e64 = np.asarray(eye, np.float64)
    z = -e64 / np.linalg.norm(e64)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    y /= np.linalg.norm(y)
    c64 = (s64 - e64) @ np.stack([x, y, z]).T
    w = np.tan(30.0 / 180 * np.pi)
    c64 = np.stack([c64[:, 0] / c64[:, 2] / w, c64[:, 1] / c64[:, 2] / w, c64[:, 2]], -1)
    out["side_proj"], out["bound_side_proj"] = cam, np.abs(cam[0] - c64).max()

    # align_to_input where the resize is the identity: a small frame (crop near two borders, mean_cent False) in full, and
    # the real geometry with mean_cent True as a strided sample plus a CRC of the whole
    info = {"rgb_newsize": (256, 192), "crop_center": np.array([40.0, 170.0]), "crop_size": np.array([150, 150])}
    out["align_small_rgb"] = ru.align_to_input(info, 192, pattern(256, 256), 150, 256, False)
    out["align_small_mask"] = ru.align_to_input(info, 192, pattern(256, 256)[:, :, 0], 150, 256, False, 0)
    info = {"rgb_newsize": (2048, 1536), "crop_center": np.array([700.0, 640.0]), "crop_size": np.array([1200, 1200])}
    big = ru.align_to_input(info, 1536, pattern(2048, 2048), 1200, 2048, True)
    out["align_mean_sample"] = big[::16, ::16].copy()
    out["align_mean_crc"] = np.int64(zlib.crc32(np.ascontiguousarray(big).tobytes()))
    out["description"] = np.array(
        "reference host-side rendering results on CPU tensors (see make_render_golden.py); align_to_input is recorded only "
        "where crop_size == train_crop_size, i.e. up to its cv2.resize, which is then the identity.  The light settings "
        "(light_args_*: ambient, directional, direction) are literals of the generator passed to the reference's "
        "lighting(): ambient and direction are what its setup_renderer / setup_side_renderer set, the directional 0.3 is what "
        "they mean to set -- they write it to an attribute the reference Renderer never reads, which would light with its "
        "constructor's 0.5.  lit_* / light64_* are therefore reference lighting() under those arguments, not a recording "
        "of the reference renderer's effective light")
    path = os.path.join(HERE, "render_host.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if k.startswith("bound_"):
            print(k, out[k])


if __name__ == "__main__":
    main()
