"""GPU: photo textures and point visibility (csrc/photo_tex.hip: chore_photo_textures_fwd, chore_point_visibility;
chore_amd.render.sample_depth / photo_textures / point_visibility, Renderer.photo_textures / vertex_visibility) against the
float64 restatement tests/photo_tex_ref.py.  The depth image is always the library's own, so no winner enters a comparison;
the texels whose decision hangs on less than the restatement's margins are left out, at most 2 % of any image."""

import numpy as np
import pytest
import torch

import photo_tex_ref as pref
from meshes import icosphere

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.1, 100.0
TOL = 5e-4        # position error <= 1e-4 px, slope of a bilinear blend of values in [0,1] <= 1 per px and axis, fp32 rounding on top


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def hip_textures(tri, depth, photo, fallback, ts, bias=pref.BIAS, align_corners=False):
    from chore_amd.render import photo_textures
    tex, vis = photo_textures(dev(tri), depth, dev(photo), dev(fallback), ts, bias, NEAR, FAR, align_corners, return_visible=True)
    assert tex.shape == tri.shape[:2] + (ts, ts, ts, 3) and vis.shape == tri.shape[:2] + (ts, ts, ts) and vis.dtype == torch.bool
    return tex.cpu().numpy(), vis.cpu().numpy()


def compare(tex, vis, ref, what):
    """visible exactly and textures within TOL outside the left-out set, which is at most 2 % of any image"""
    keep = ~ref["left_out"]
    share = ref["left_out"].reshape(len(keep), -1).mean(1)
    err = np.abs(tex - ref["textures"]).max(-1)
    print(what, "left out per image:", np.round(share, 4).tolist(), "visible mismatches:", int((vis != ref["visible"])[keep].sum()),
          "max colour error:", float(err[keep].max()), "(left-out texels: %g)" % float(err[~keep].max() if (~keep).any() else 0))
    assert (share <= pref.LEFT_OUT_CAP).all(), share
    assert np.array_equal(vis[keep], ref["visible"][keep])
    assert err[keep].max() <= TOL


@pytest.fixture(scope="module")
def random_case():
    """test 1's inputs and, per S, the library's depth image (device tensor and host copy), computed once"""
    from chore_amd.render import sample_depth
    tri = pref.random_tri(0)
    photo, fallback = pref.random_inputs(tri)
    depth = {S: sample_depth(dev(tri), S, NEAR, FAR) for S in sorted({S for S, _ in pref.CASES})}
    return tri, photo, fallback, depth


@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("S,ts", pref.CASES)
def test_random_meshes(random_case, S, ts, align_corners):
    """1: B = 3, 80 triangles, photo 48 x 64, against the restatement on the library's depth image"""
    tri, photo, fallback, depth = random_case
    d = depth[S]
    assert d.shape == (3, S, S) and float(d.max()) == FAR and float(d.min()) > NEAR
    ref = pref.photo_textures(tri, d.cpu().numpy(), photo, fallback, ts, NEAR, FAR, pref.BIAS, align_corners)
    sh = pref.shares(ref)
    print({k: np.round(v, 4).tolist() for k, v in sh.items()})
    # every class is populated; image 1's triangles are scaled into |u|, |v| < 0.36: all in view and inside the photo's rows
    assert all((sh[k] > 0).all() for k in ("in_view", "visible", "occluded"))
    assert (sh["outside_photo"][[0, 2]] > 0).all() and (sh["in_view"][[0, 2]] < 1).all()
    tex, vis = hip_textures(tri, d, photo, fallback, ts, pref.BIAS, align_corners)
    compare(tex, vis, ref, "S=%d ts=%d align_corners=%s" % (S, ts, align_corners))


def test_sample_depth_is_the_renderers(random_case):
    """the depth image is chore_render_fwd's at ssaa 1 with the rows reversed, bit for bit"""
    from chore_amd.render import rasterize_rgbad
    tri, _, _, depth = random_case
    t = dev(tri)
    tex = torch.ones(tri.shape[0], tri.shape[1], 2, 2, 2, 3, device="cuda")
    for S, d in depth.items():
        assert torch.equal(d.flip(1), rasterize_rgbad(t, tex, None, S, False, NEAR, FAR)["depth"]), S


def test_exact_properties(random_case):
    """2: no tolerance: a constant photo, the two extreme biases, texel_visible = NULL, two calls"""
    from chore_amd.render import photo_textures
    tri, photo, fallback, depth = random_case
    S, ts = 61, 5
    d = depth[S]
    t, fb = dev(tri), dev(fallback)
    tex, vis = hip_textures(tri, d, photo, fallback, ts)
    again = hip_textures(tri, d, photo, fallback, ts)
    assert np.array_equal(tex, again[0]) and np.array_equal(vis, again[1])                          # two calls are bit-equal
    assert torch.equal(photo_textures(t, d, dev(photo), fb, ts, pref.BIAS, NEAR, FAR), torch.as_tensor(tex).cuda())    # visible = NULL
    assert vis.any() and not vis.all()
    # constant photo: only that colour (a + (b - a) f is a when the taps are equal) or the fallback
    const = np.broadcast_to(np.float32([0.25, 0.5, 0.75]).reshape(1, 3, 1, 1), photo.shape)
    ctex, cvis = hip_textures(tri, d, const, fallback, ts)
    is_fb = (ctex == fallback[:, :, None, None, None, :]).all(-1)
    is_photo = (ctex == np.float32([0.25, 0.5, 0.75])).all(-1)
    assert (is_fb | is_photo).all() and is_photo.any() and np.array_equal(cvis, vis)
    assert is_fb[~vis].all() and not (is_photo & ~vis).any()
    # bias = 1e9: every texel in view with near < z < far is visible; bias = -1e9: none is, and textures == fallback
    ref = pref.photo_textures(tri, d.cpu().numpy(), photo, fallback, ts, NEAR, FAR, 1e9)
    _, allvis = hip_textures(tri, d, photo, fallback, ts, bias=1e9)
    keep = ~ref["left_out"]
    assert np.array_equal(allvis[keep], ref["in_view"][keep]) and (allvis | ~vis).all() and allvis.sum() > vis.sum()
    ntex, nvis = hip_textures(tri, d, photo, fallback, ts, bias=-1e9)
    assert not nvis.any() and np.array_equal(ntex, np.broadcast_to(fallback[:, :, None, None, None, :], ntex.shape))


@pytest.mark.parametrize("S,ts", pref.CASES)
def test_points_against_texels(random_case, S, ts):
    """3: point_visibility at the three vertices of every face equals texel_visible at the one-hot texels, exactly"""
    from chore_amd.render import point_visibility
    tri, photo, fallback, depth = random_case
    B, Fn = tri.shape[:2]
    _, vis = hip_textures(tri, depth[S], photo, fallback, ts)
    pv = point_visibility(dev(tri.reshape(B, Fn * 3, 3)), depth[S], pref.BIAS, NEAR, FAR)
    assert pv.dtype == torch.int32 and pv.shape == (B, Fn * 3)
    pv = pv.cpu().numpy().reshape(B, Fn, 3)
    corner = np.stack([vis[:, :, ts - 1, 0, 0], vis[:, :, 0, ts - 1, 0], vis[:, :, 0, 0, ts - 1]], -1)
    assert set(np.unique(pv)) == {0, 1} and np.array_equal(pv.astype(bool), corner)
    want, left = pref.point_visibility(tri.reshape(B, Fn * 3, 3), depth[S].cpu().numpy(), NEAR, FAR, pref.BIAS)
    assert np.array_equal(pv.reshape(B, -1).astype(bool)[~left], want[~left]) and left.mean() <= pref.LEFT_OUT_CAP


SPHERE_R, WALL_Z, WALL_HALF = 0.5, 1.0, 1.5
OFF = np.array([0.0137, -0.0213, 0.0])        # off the axis: a symmetric scene puts whole rows of texels exactly between two samples


@pytest.fixture(scope="module")
def closed_scene():
    """an icosphere next to the origin in front of a two-triangle wall, seen by a look_at camera on the -z axis"""
    v, f = icosphere(2, SPHERE_R, OFF)
    wall = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float64) * WALL_HALF + [0, 0, WALL_Z] + OFF
    verts = np.concatenate([v, wall])[None].astype(np.float32)
    faces = np.concatenate([f, np.array([[0, 1, 2], [0, 2, 3]]) + len(v)])[None].astype(np.int32)
    return verts, faces, len(f)


def test_closed_mesh(closed_scene):
    """4: B = 1, S = 96, through Renderer.photo_textures / vertex_visibility with fill_back: the wall behind the sphere and the
    sphere's far hemisphere are not visible; the restatement under the same cap; render() shows the photo on the near side"""
    from chore_amd.render import Renderer, sample_depth, vertices_to_faces
    verts, faces, n_sphere = closed_scene
    S, ts = 96, 4
    r = Renderer(image_size=S, camera_mode="look_at", fill_back=True)
    r.light_intensity_ambient, r.light_intensity_directional = 1.0, 0.0                   # the light factor is 1 for every face
    V, Fc = dev(verts), dev(faces, torch.int32)
    photo = np.zeros((1, 3, S, S), np.float32)
    photo[:, 0] = 1.0                                                                       # red
    photo[:, 1] = np.linspace(0, 0.5, S, dtype=np.float32)[None, None, :]                    # green grows with x
    blue = np.float32([0, 0, 1])
    tex, vis = r.photo_textures(V, Fc, dev(photo), blue, ts, return_visible=True)
    assert tex.shape == (1, faces.shape[1], ts, ts, ts, 3)
    tex_np, vis_np = tex.cpu().numpy(), vis.cpu().numpy()
    # the restatement on the projected triangles the renderer uses and the library's depth image of both windings
    ndc = r.transform(V)
    tri = vertices_to_faces(ndc, Fc)
    depth = sample_depth(vertices_to_faces(ndc, torch.cat((Fc, Fc.flip(-1)), 1)), S, r.near, r.far)
    ref = pref.photo_textures(tri.cpu().numpy(), depth.cpu().numpy(), photo, np.broadcast_to(blue, (1, faces.shape[1], 3)), ts,
                              r.near, r.far, 0.02)
    compare(tex_np, vis_np, ref, "closed mesh")
    # geometry, with margins of more than a sample: texel positions in the world are the weights applied to the vertices
    w = pref.texel_weights(ts)                                                                 # (ts,ts,ts,3)
    pos = np.einsum("ijkc,fcd->fijkd", w, verts[0][faces[0]].astype(np.float64))               # (F,ts,ts,ts,3)
    sphere, wall = pos[:n_sphere], pos[n_sphere:]
    assert not vis_np[0, :n_sphere][sphere[..., 2] > 0.15].any()                               # the far hemisphere
    assert vis_np[0, :n_sphere][sphere[..., 2] < -0.4].all()                                   # the near cap
    eye_d = -r.eye[2]
    rim = SPHERE_R / np.sqrt(eye_d ** 2 - SPHERE_R ** 2) * (eye_d + WALL_Z)                    # radius of the sphere's shadow on the wall
    shadow = OFF[:2] * (eye_d + WALL_Z) / eye_d                                                # its centre: the sphere's, seen from the eye
    rad = np.hypot(wall[..., 0] - shadow[0], wall[..., 1] - shadow[1])
    in_view = np.abs(wall[..., :2]).max(-1) < 0.95 * np.tan(np.radians(30)) * (eye_d + WALL_Z)
    assert (rad < 0.9 * rim).any() and not vis_np[0, n_sphere:][rad < 0.9 * rim].any()
    assert (in_view & (rad > 1.1 * rim)).any() and vis_np[0, n_sphere:][in_view & (rad > 1.1 * rim)].all()
    # vertices: the sphere's poles towards and away from the camera, and the restatement
    vv = r.vertex_visibility(V, Fc)
    assert vv.shape == (1, verts.shape[1]) and vv.dtype == torch.int32
    vv = vv.cpu().numpy()[0].astype(bool)
    assert not vv[:-4][verts[0, :-4, 2] > 0.15].any() and vv[:-4][verts[0, :-4, 2] < -0.4].all()
    want, left = pref.point_visibility(ndc.cpu().numpy(), depth.cpu().numpy(), r.near, r.far, 0.02)
    assert np.array_equal(vv[~left[0]], want[0][~left[0]])
    # the rendering: red with the photo's green ramp where the camera sees the scene, never the fallback's blue
    rgb, _, alpha = r.render(V, Fc, tex)
    rgb, alpha = rgb.cpu().numpy()[0], alpha.cpu().numpy()[0]
    mid = S // 2
    assert alpha[mid, mid] == 1 and rgb[0, mid, mid] > 0.95 and rgb[2, mid, mid] < 0.05
    # the wall spans |u| < 0.696: columns 19 and 77 are u = -0.6 and 0.6 on it, where the ramp is 0.10 and 0.40
    assert abs(rgb[1, mid, mid] - 0.25) < 0.03 and abs(rgb[1, mid, 19] - 0.10) < 0.05 and abs(rgb[1, mid, 77] - 0.40) < 0.05
    # blue shows only in a ring inside the sphere's limb, where the surface is steeper than depth_bias per half sample
    covered = alpha == 1
    assert covered.mean() > 0.4 and (rgb[2][covered] < 0.5).mean() > 0.9


def test_refusals(random_case):
    """5: ts = 1 and 17, Hp > Wp, S = 4097 and NULL pointers return CHORE_EINVAL before anything is launched; ValueError from Python"""
    from chore_amd import _lib
    from chore_amd.render import photo_textures, point_visibility, sample_depth
    tri, photo, fallback, depth = random_case
    L, h = _lib.lib, _lib.handle(0)
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()

    def tex_call(tri_p=p, B=1, F=1, ts=2, S=8, Hp=4, Wp=4, out=p):
        return L.chore_photo_textures_fwd(h, tri_p, p, p, p, B, F, ts, S, Hp, Wp, NEAR, FAR, 0.02, 0, out, None, st)
    EINVAL = tex_call(tri_p=None)
    assert EINVAL != 0 and b"chore_photo_textures_fwd" in L.chore_last_error(h)
    assert tex_call() == 0
    for kw in (dict(ts=1), dict(ts=17), dict(Hp=5, Wp=4), dict(S=4097), dict(S=0), dict(B=0), dict(F=0), dict(Hp=0), dict(Wp=0, Hp=0),
               dict(out=None)):
        assert tex_call(**kw) == EINVAL, kw
    assert L.chore_point_visibility(h, p, p, 1, 1, 8, NEAR, FAR, 0.02, p, st) == 0
    for args in ((None, p, 1, 1, 8, p), (p, None, 1, 1, 8, p), (p, p, 1, 1, 8, None), (p, p, 0, 1, 8, p), (p, p, 1, 0, 8, p),
                 (p, p, 1, 1, 4097, p), (p, p, 1, 1, 0, p)):
        assert L.chore_point_visibility(h, args[0], args[1], args[2], args[3], args[4], NEAR, FAR, 0.02, args[5], st) == EINVAL, args
    torch.cuda.synchronize()
    assert not buf[64:].any()                                   # the two valid calls wrote 24 floats and one int at most
    t, ph, fb, d = dev(tri), dev(photo), dev(fallback), depth[61]
    for ts in (1, 17):
        with pytest.raises(ValueError):
            photo_textures(t, d, ph, fb, ts)
    with pytest.raises(ValueError):
        photo_textures(t, d, ph.transpose(2, 3), fb)            # Hp > Wp
    with pytest.raises(ValueError):
        photo_textures(t, torch.zeros(3, 4097, 4097, device="cuda"), ph, fb)
    with pytest.raises(ValueError):
        sample_depth(t, 4097)
    with pytest.raises(ValueError):
        point_visibility(t.reshape(3, -1, 3), d[:2])
    with pytest.raises(RuntimeError):
        photo_textures(t.cpu(), d, ph, fb)
