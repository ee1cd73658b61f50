"""GPU: the HIP colour / depth rasteriser (chore_render_fwd), chore_amd.render.Renderer and chore_amd.utils.render_utils
against the silhouette rasteriser (chore_silhouette_fwd), the numpy restatements (oracle/silhouette.py, tests/render_ref.py)
and known answers."""
import numpy as np
import pytest
import torch

import render_ref
from meshes import icosphere
from oracle import silhouette as osil

pytestmark = pytest.mark.gpu

NEAR, FAR, TEX_EPS = 0.1, 100.0, 1e-3


def random_tri(seed=0, B=3, V=30, Fn=40):
    """projected triangles in the style of tests/test_gpu_silhouette.py random_mesh: in and around the view, small triangles
    in image 1, degenerate vertices in image 2, both windings"""
    rs = np.random.RandomState(seed)
    v = np.concatenate([rs.uniform(-1.2, 1.2, (B, V, 2)), rs.uniform(0.5, 4.0, (B, V, 1))], -1).astype(np.float32)
    f = np.stack([np.stack([rs.choice(V, 3, replace=False) for _ in range(Fn)]) for _ in range(B)]).astype(np.int64)
    v[1, :, :2] *= 0.3
    v[2, :5] = 0.0
    return osil.vertices_to_faces(v, osil.fill_back(f)), rs


def hip_render(tri, tex, light, size, ssaa, background=(0, 0, 0), near=NEAR, far=FAR):
    from chore_amd.render import rasterize_rgbad
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float32)).cuda()     # noqa: E731
    out = rasterize_rgbad(t(tri), t(tex), t(light), size, ssaa == 2, near, far, TEX_EPS, background, return_index=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def hip_silhouette_index(tri, S):
    from chore_amd.recon.obj_pose_roi import _RasterizeFn
    t = tri if torch.is_tensor(tri) else torch.from_numpy(np.asarray(tri, np.float32))
    _, fim = _RasterizeFn.apply(t.cuda(), S)
    return fim.cpu().numpy()


def white(tri, ts=2):
    return np.ones(tri.shape[:2] + (ts, ts, ts, 3), np.float32)


def demo_scene():
    """the body-sized ellipsoid at 2.2 m and a sphere of radius 0.3 beside it: (verts (V,3), faces (F,3), F of the body)"""
    from chore_amd.utils.synth import uv_ellipsoid
    bv, bf = uv_ellipsoid(center=(0.0, 0.0, 2.2))
    sv, sf = icosphere(3, 0.3, (0.6, 0.0, 2.2))
    return (np.concatenate([bv, sv]).astype(np.float32), np.concatenate([bf, sf + len(bv)]).astype(np.int64), len(bf))


def test_winner_per_sample_random_meshes():
    """1a: sample_face_index is bit-equal to the silhouette restatement and to chore_silhouette_fwd at size * ssaa"""
    tri, _ = random_tri(0)
    out = hip_render(tri, white(tri), None, 64, 2)
    fim_o = render_ref.winners(tri, 128)
    assert 0.05 < (fim_o >= 0).mean() < 0.95
    assert np.array_equal(out["face_index"], fim_o)
    assert np.array_equal(out["face_index"], hip_silhouette_index(tri, 128))


def test_winner_per_sample_tail_batch_bins_and_zero_area():
    """1c: a size that is no multiple of the tile (200 px at 2x = 400 samples: partly filled workgroups, 2 x 2 coarse bins)
    with B = 2, and zero-area triangles (collinear or repeated vertices, long enough to cross tiles and bins) in the list:
    winners equal chore_silhouette_fwd at 400 and the restatement, exactly; the resolved alpha agrees with them"""
    rs = np.random.RandomState(11)
    B, V, Fn, size = 2, 40, 60, 200
    v = np.concatenate([rs.uniform(-1.2, 1.2, (B, V, 2)), rs.uniform(0.5, 4.0, (B, V, 1))], -1).astype(np.float32)
    f = np.stack([np.stack([rs.choice(V, 3, replace=False) for _ in range(Fn)]) for _ in range(B)]).astype(np.int64)
    tri = osil.vertices_to_faces(v, f)
    # zero-area triangles: a + t (b - a) on sample centres and on dyadic coordinates (exact products), and a repeated vertex
    S = 2 * size
    deg = []
    for _ in range(12):
        a = (2 * rs.randint(20, 380, 2) + 1 - S) / S
        d = rs.randint(-6, 7, 2) * 2 / S
        z = rs.uniform(0.5, 4.0, 3)
        deg.append([[a[0], a[1], z[0]], [a[0] + 3 * d[0], a[1] + 3 * d[1], z[1]], [a[0] + 8 * d[0], a[1] + 8 * d[1], z[2]]])
    for _ in range(6):
        a, b = rs.choice([-0.75, -0.5, -0.25, 0.0, 0.25, 0.5], 2), rs.choice([-0.5, 0.0, 0.125, 0.5, 0.75], 2)
        deg.append([[a[0], a[1], 1.5], [(a[0] + b[0]) / 2, (a[1] + b[1]) / 2, 2.0], [b[0], b[1], 2.5]])
        deg.append([[a[0], a[1], 1.5], [a[0], a[1], 1.5], [b[0], b[1], 2.5]])
    deg = np.broadcast_to(np.asarray(deg, np.float32), (B, len(deg), 3, 3))
    regular = np.ascontiguousarray(np.concatenate([tri, tri[:, :, ::-1]], 1))
    assert np.array_equal(hip_render(regular, white(regular), None, size, 2)["face_index"], render_ref.winners(regular, S))
    # with the zero-area triangles the yardstick is the silhouette kernel alone: the numpy restatement clips NaN weights
    # to NaN where the kernels' fmin / fmax give 0, so it is no authority on triangles whose inverse does not exist
    tri = np.concatenate([tri, deg], 1)
    tri = np.ascontiguousarray(np.concatenate([tri, tri[:, :, ::-1]], 1))
    out = hip_render(tri, white(tri), None, size, 2)
    fim = out["face_index"]
    assert fim.shape == (B, S, S)
    assert np.array_equal(fim, hip_silhouette_index(tri, S))
    assert all(0.05 < (fim[b] >= 0).mean() < 0.95 for b in range(B)) and not np.array_equal(fim[0], fim[1])
    cover = (fim >= 0).astype(np.float32)
    want = ((((cover[:, 0::2, 0::2] + cover[:, 0::2, 1::2]) + cover[:, 1::2, 0::2]) + cover[:, 1::2, 1::2]) * 0.25)[:, ::-1]
    assert out["alpha"].shape == (B, size, size) and np.array_equal(out["alpha"], want)
    one = hip_render(tri, white(tri), None, S - 3, 1)          # ssaa = 1 at an odd size, against the silhouette kernel
    assert np.array_equal(one["face_index"], hip_silhouette_index(tri, S - 3))


def test_winner_per_sample_demo_view():
    """1b: the demo view, 2048 px at 2x super-sampling (30 112 triangles, 4096^2 samples), against chore_silhouette_fwd"""
    from chore_amd.recon.obj_pose_roi import vertices_to_faces
    from chore_amd.utils.render_utils import setup_renderer
    v, f, nbody = demo_scene()
    r = setup_renderer(image_size=2048)
    vt = torch.from_numpy(v)[None].cuda()
    ft = torch.from_numpy(f)[None].cuda()
    f2 = torch.cat((ft, ft.flip(-1)), 1)
    tri = vertices_to_faces(r.transform(vt), f2)
    Fn = f.shape[0]
    assert tri.shape[1] == 30112
    out = hip_render(tri.cpu().numpy(), white(tri), None, 2048, 2)
    fim = out["face_index"]
    assert np.array_equal(fim, hip_silhouette_index(tri, 4096))
    share = (out["alpha"] > 0).mean()
    print("covered share of the 2048^2 frame:", share)
    assert 0.02 < share < 0.5
    won = np.unique(fim[fim >= 0]) % Fn
    assert (won < nbody).any() and (won >= nbody).any()


def test_values_against_restatement():
    """2: rgb / depth / alpha with the kernel's own winners against tests/render_ref.py in float64.  Allowed: 4 x the largest
    difference between the restatement evaluated in float32 and in float64, per output.  Measured bounds (seed 0, B = 3,
    80 triangles per image, ts = 4, 64 px at 2x; 4 x the float32 / float64 difference): rgb 1.85e-5, depth 2.24e-5 (slivers
    with an ill-conditioned inverse dominate both), alpha 0 (exact).  The kernel's own error against float64 on an MI355X was
    4.6e-6 / 5.6e-6 / 0, i.e. it reproduces the float32 restatement."""
    tri, rs = random_tri(0)
    B, Fn = tri.shape[:2]
    tex = rs.uniform(0, 1, (B, Fn, 4, 4, 4, 3)).astype(np.float32)
    light = rs.uniform(0.2, 1.2, (B, Fn, 3)).astype(np.float32)
    bg = (0.1, 0.5, 0.9)
    out = hip_render(tri, tex, light, 64, 2, bg)
    fim = out["face_index"]
    r32 = render_ref.render(tri, tex, light, fim, 2, NEAR, FAR, TEX_EPS, bg, np.float32)
    r64 = render_ref.render(tri, tex, light, fim, 2, NEAR, FAR, TEX_EPS, bg, np.float64)
    for name, a32, a64 in zip(("rgb", "depth", "alpha"), r32, r64):
        bound = 4 * np.abs(a32.astype(np.float64) - a64).max()
        err = np.abs(out[name].astype(np.float64) - a64).max()
        print("%s: bound %.3e  kernel error %.3e" % (name, bound, err))
        assert out[name].shape == a64.shape
        assert err <= bound, (name, err, bound)
    assert set(np.unique(out["alpha"]).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    assert len(np.unique(out["alpha"])) >= 4


def square(x0, x1, y0, y1, z, reverse=None):
    """two triangles; reverse = None: both windings, False / True: one of them"""
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    t = np.array([[a, b, c], [a, c, d]], np.float32)
    if reverse is None:
        return np.concatenate([t, t[:, ::-1]])
    return t[:, ::-1].copy() if reverse else t


def uniform_tex(colors, ts=2):
    c = np.asarray(colors, np.float32)
    return np.broadcast_to(c[:, None, None, None, :], (len(c), ts, ts, ts, 3)).copy()


C1, L1 = np.array([0.9, 0.5, 0.2], np.float32), np.array([0.8, 1.1, 0.6], np.float32)
C2, L2 = np.array([0.1, 0.7, 0.4], np.float32), np.array([1.2, 0.5, 0.9], np.float32)
BG = np.array([0.3, 0.2, 0.7], np.float32)
SQ = (-62 / 128, 0.5, -0.25, 0.75)


def test_known_square():
    """3a: alpha in {0, 0.5, 1} on columns 16-47, rows 8-39 (the image is flipped as the reference flips it)"""
    tri = square(*SQ, 2.0)[None]
    out = hip_render(tri, uniform_tex([C1] * 4)[None], np.tile(L1, (1, 4, 1)), 64, 2, BG)
    alpha, rgb, depth = out["alpha"][0], out["rgb"][0], out["depth"][0]
    want = np.zeros((64, 64), np.float32)
    want[8:40, 17:48] = 1.0
    want[8:40, 16] = 0.5
    assert np.array_equal(alpha, want)
    full, half, none = want == 1, want == 0.5, want == 0
    lit = C1 * L1
    assert np.abs(rgb[:, full] - lit[:, None]).max() < 1e-6
    assert np.abs(rgb[:, half] - (0.5 * lit + 0.5 * BG)[:, None]).max() < 1e-6
    assert np.abs(rgb[:, none] - BG[:, None]).max() == 0
    assert np.abs(depth[full] - 2.0).max() < 1e-5
    assert np.abs(depth[half] - (2.0 + FAR) / 2).max() < 1e-5
    assert np.all(depth[none] == np.float32(FAR))


def test_known_nearer_square_wins():
    """3b: a nearer, smaller square of another colour wins where it covers"""
    tri = np.concatenate([square(*SQ, 2.0), square(0.0, 0.25, 0.0, 0.25, 1.0)])[None]
    tex = uniform_tex([C1] * 4 + [C2] * 4)[None]
    light = np.concatenate([np.tile(L1, (4, 1)), np.tile(L2, (4, 1))])[None]
    out = hip_render(tri, tex, light, 64, 2, BG)
    rgb, depth = out["rgb"][0], out["depth"][0]
    near_sq = np.zeros((64, 64), bool)
    near_sq[24:32, 32:40] = True
    assert np.abs(rgb[:, near_sq] - (C2 * L2)[:, None]).max() < 1e-6
    assert np.abs(depth[near_sq] - 1.0).max() < 1e-5
    far_sq = np.zeros((64, 64), bool)
    far_sq[8:40, 17:48] = True
    far_sq &= ~near_sq
    assert np.abs(rgb[:, far_sq] - (C1 * L1)[:, None]).max() < 1e-6
    assert np.abs(depth[far_sq] - 2.0).max() < 1e-5


@pytest.mark.parametrize("z", [NEAR / 2, 2 * FAR])
def test_known_outside_near_far(z):
    """3c: nothing is drawn in front of near or beyond far"""
    out = hip_render(square(*SQ, z)[None], uniform_tex([C1] * 4)[None], None, 64, 2, BG)
    assert np.all(out["alpha"] == 0) and np.all(out["depth"] == np.float32(FAR)) and np.all(out["face_index"] == -1)
    assert np.all(out["rgb"][0] == BG[:, None, None])


def test_known_back_faces():
    """3d: one winding alone is culled when seen from behind; the list with both windings is drawn"""
    drawn = []
    for rev in (False, True):
        out = hip_render(square(*SQ, 2.0, reverse=rev)[None], uniform_tex([C1] * 2)[None], None, 64, 2, BG)
        drawn.append(bool((out["alpha"] > 0).any()))
        if not drawn[-1]:
            assert np.all(out["rgb"][0] == BG[:, None, None])
    assert sorted(drawn) == [False, True]
    out = hip_render(square(*SQ, 2.0)[None], uniform_tex([C1] * 4)[None], None, 64, 2, BG)
    assert (out["alpha"] > 0).sum() == 32 * 32


def test_ssaa1_equals_unaveraged_samples():
    """3e: ssaa = 1 at 128 px gives the samples that ssaa = 2 at 64 px averages"""
    tri, rs = random_tri(3)
    B, Fn = tri.shape[:2]
    tex = rs.uniform(0, 1, (B, Fn, 4, 4, 4, 3)).astype(np.float32)
    light = rs.uniform(0.2, 1.2, (B, Fn, 3)).astype(np.float32)
    one = hip_render(tri, tex, light, 128, 1, BG)
    two = hip_render(tri, tex, light, 64, 2, BG)
    assert np.array_equal(one["face_index"], two["face_index"])

    def pool(a):        # a (..., 128, 128) flipped rows: image row 2r+1 is the lower sample row of pixel row r
        return (((a[..., 1::2, 0::2] + a[..., 1::2, 1::2]) + a[..., 0::2, 0::2]) + a[..., 0::2, 1::2]) * np.float32(0.25)
    for k in ("rgb", "depth", "alpha"):
        assert np.array_equal(pool(one[k]), two[k]), k


def test_nothing_dropped():
    """4: 6 000 small triangles of distinct depths whose boxes all meet one 16x16-pixel tile, and a few hundred elsewhere:
    every sample's winner equals chore_silhouette_fwd's (the reference's 4x4 blocks would keep 512 ids and lose the rest)"""
    rs = np.random.RandomState(5)
    n, m, S = 6000, 300, 128

    def tris(count, lo, hi):
        c = rs.uniform(lo, hi, (count, 1, 2))                        # centres in sample coordinates
        p = c + rs.uniform(-3, 3, (count, 3, 2))
        xy = (2 * p + 1 - S) / S
        return xy
    xy = np.concatenate([tris(n, 36, 60), tris(m, 2, 126)])          # tile (1,1) of 32x32 samples: 32..63
    z = 1.0 + rs.permutation(n + m) * 1e-4
    tri = np.concatenate([xy, np.broadcast_to(z[:, None, None], (n + m, 3, 1))], -1).astype(np.float32)[None]
    flip = rs.rand(n + m) < 0.5
    tri[0, flip] = tri[0, flip][:, ::-1]
    tri = np.concatenate([tri, tri[:, :, ::-1]], 1)
    out = hip_render(tri, white(tri), None, 64, 2)
    fim = out["face_index"]
    assert np.array_equal(fim, hip_silhouette_index(tri, S))
    in_tile = np.unique(fim[0, 32:64, 32:64])
    assert (in_tile >= 0).sum() > 100 and (fim[0, 32:64, 32:64] >= 0).mean() > 0.7
    assert (in_tile % (n + m) >= 512).any()


def _light64(v, f2, ia, idir, direction):
    """the fixture formula of lighting.py in float64: per face of the doubled list"""
    t = v.astype(np.float64)[f2]
    nrm = np.cross(t[:, 0] - t[:, 1], t[:, 2] - t[:, 1])
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-5)
    return ia + idir * np.maximum(nrm @ np.asarray(direction, np.float64), 0.0)


def test_lighting_end_to_end():
    """5: Renderer.render on a sphere under setup_renderer's light: the colour of every covered pixel is the texture colour
    times the light of the winning face; with no directional light the render is flat"""
    from chore_amd.utils.render_utils import setup_renderer
    v, f = icosphere(2, 0.5, (0.1, -0.1, 2.2))
    v, f = v.astype(np.float32), f.astype(np.int64)
    r = setup_renderer(image_size=256)
    r.anti_aliasing = False
    vt, ft = torch.from_numpy(v)[None].cuda(), torch.from_numpy(f)[None].cuda()
    tex = torch.from_numpy(uniform_tex([C1] * len(f), 4))[None].cuda()
    out = r._rasterize(vt, ft, tex, (None,) * 5, return_index=True)
    rgb, depth, alpha = r.render(vt, ft, tex)
    assert torch.equal(rgb, out["rgb"]) and torch.equal(alpha, out["alpha"]) and torch.equal(depth, out["depth"])
    assert rgb.shape == (1, 3, 256, 256) and depth.shape == (1, 256, 256) and alpha.shape == (1, 256, 256)
    fim = out["face_index"][0].cpu().numpy()[::-1]                  # to image rows
    f2 = np.concatenate([f, f[:, ::-1]])
    light = _light64(v, f2, 0.4, 0.3, [1, 0.5, 1])
    hit = fim >= 0
    assert 0.02 < hit.mean() < 0.5
    want = C1[None, :].astype(np.float64) * light[fim[hit]][:, None]
    got = rgb[0].cpu().numpy()[:, hit].T
    assert np.abs(got - want).max() < 1e-5
    assert np.ptp(light[fim[hit]]) > 0.05 and light[fim[hit]].min() >= 0.4 and light[fim[hit]].max() <= 0.85
    assert np.all(rgb[0].cpu().numpy()[:, ~hit] == 1.0)           # setup_renderer's white background
    r.light_intensity_directional = 0
    flat = r.render_rgb(vt, ft, tex)[0].cpu().numpy()[:, hit].T
    assert np.abs(flat - 0.4 * C1[None, :]).max() < 1e-6


def _meshes():
    from chore_amd.utils.render_utils import Mesh
    from chore_amd.utils.synth import uv_ellipsoid
    bv, bf = uv_ellipsoid(center=(0.0, 0.0, 2.2))
    sv, sf = icosphere(3, 0.3, (0.6, 0.0, 2.2))
    return Mesh(v=bv, f=bf), Mesh(v=sv, f=sf)


def test_nrwrapper_front_and_side():
    """6: NrWrapper at 512 px: image range, mask = alpha != 0, body and object pixels in their colours times a light factor
    in [0.4, 0.85]; the side view is non-empty and inside the frame"""
    from chore_amd.utils import render_utils as ru
    body, obj = _meshes()
    nrw = ru.NrWrapper(image_size=512)
    rend, mask = nrw.render_meshes(nrw.front_renderer, [body, obj])
    assert rend.shape == (512, 512, 3) and rend.dtype == np.float32 and rend.min() >= 0 and rend.max() <= 1
    assert mask.shape == (512, 512) and mask.dtype == bool
    verts, faces, texts = nrw.prepare_render([body, obj])
    _, _, alpha = nrw.front_renderer.render(verts, faces, texts)
    alpha = alpha[0].cpu().numpy()
    assert np.array_equal(mask, alpha != 0) and 0.02 < mask.mean() < 0.5
    px = rend[alpha == 1].astype(np.float64)
    kinds = []
    for color in ru.SMPL_OBJ_COLOR_LIST:
        ratio = px / np.asarray(color)[None, :]
        kinds.append((ratio.max(1) - ratio.min(1) < 1e-4, ratio.mean(1)))
    (is_body, fb), (is_obj, fo) = kinds
    assert np.all(is_body | is_obj) and is_body.sum() > 1000 and is_obj.sum() > 1000
    for sel, fac in ((is_body, fb), (is_obj, fo)):
        assert fac[sel].min() >= 0.4 - 1e-4 and fac[sel].max() <= 0.85 + 1e-4
    assert np.all(rend[~mask] == 1.0)
    # the body is left of the object in the image (x grows to the right under the Kinect intrinsics)
    cols = np.nonzero(alpha == 1)[1]
    assert cols[is_body].mean() < cols[is_obj].mean()
    # side view
    faces, texts, sverts = nrw.prepare_side_rend([body, obj], maxd=1.8)
    side, smask = nrw.render(ru.setup_side_renderer(2.0, 0., 90.), sverts, faces, texts)
    assert side.shape == (640, 640, 3) and smask.shape == (640, 640)
    assert smask.mean() > 0.02
    assert not (smask[0].any() or smask[-1].any() or smask[:, 0].any() or smask[:, -1].any())
    assert abs(body.v[:, 2].mean() - 2.2) < 1e-6                   # the caller's meshes are not modified


def test_render_fit_views():
    """6: the demo's rendering tail from decoded arrays: shapes, and the photo is untouched outside the mask"""
    from chore_amd.utils import render_utils as ru
    body, obj = _meshes()
    rs = np.random.RandomState(9)
    rgb = rs.randint(0, 256, (1536, 2048, 3)).astype(np.uint8)
    crop_info = {"rgb_newsize": (2048, 1536), "crop_center": np.array([1008.0, 995.0]), "crop_size": np.array([1200, 1200])}
    nrw = ru.NrWrapper(image_size=2048)
    overlap, side = ru.render_fit_views(rgb, crop_info, body, obj, 1200, nrwrapper=nrw)
    assert overlap.shape == (1536, 2048, 3) and overlap.dtype == np.uint8
    assert side.shape == (640, 640, 3) and side.dtype == np.uint8
    rend, mask = nrw.render_meshes(nrw.front_renderer, [body, obj])
    m = ru.align_to_input(crop_info, 1536, (mask * 255).astype(np.uint8), 1200, 2048, True, 0) > 127
    assert 0.02 < m.mean() < 0.5
    assert np.array_equal(overlap[~m], rgb[~m])
    r = ru.align_to_input(crop_info, 1536, (rend * 255).astype(np.uint8), 1200, 2048, True)
    assert np.array_equal(overlap[m], r[m])
    assert (side < 255).any()


def test_render_fit_views_with_resizes():
    """6: the case of a real demo run: the photo is not at rgb_newsize and the loader's crop is not load_size, so the photo,
    the rendering and the 2-D mask all go through ImagePrep.resize (chore_prep_resize_u8) and back"""
    from chore_amd.utils import render_utils as ru
    body, obj = _meshes()
    rs = np.random.RandomState(10)
    rgb = rs.randint(0, 256, (768, 1024, 3)).astype(np.uint8)
    crop_info = {"rgb_newsize": (2048, 1536), "crop_center": np.array([1100.0, 800.0]), "crop_size": np.array([900, 900])}
    nrw = ru.NrWrapper(image_size=2048)
    overlap, side = ru.render_fit_views(rgb, crop_info, body, obj, 1200, nrwrapper=nrw)
    assert overlap.shape == (768, 1024, 3) and overlap.dtype == np.uint8
    assert side.shape == (640, 640, 3) and side.dtype == np.uint8
    rend, mask = nrw.render_meshes(nrw.front_renderer, [body, obj])
    m2 = ru.align_to_input(crop_info, 1536, (mask * 255).astype(np.uint8), 1200, 2048, True, 0)
    r3 = ru.align_to_input(crop_info, 1536, (rend * 255).astype(np.uint8), 1200, 2048, True)
    assert m2.shape == (1536, 2048) and m2.dtype == np.uint8 and r3.shape == (1536, 2048, 3) and r3.dtype == np.uint8
    m = m2 > 127
    # the window of 1200 px around the mean crop centre shrinks to 900 px around the crop centre: the covered share
    # shrinks by about (900 / 1200)^2, and everything covered lies inside the pasted square
    full = ru.align_to_input(dict(crop_info, crop_size=np.array([1200, 1200])), 1536, (mask * 255).astype(np.uint8), 1200,
                             2048, True, 0) > 127
    assert 0.45 < m.sum() / full.sum() < 0.68
    ys, xs = np.nonzero(m)
    assert xs.min() >= 1100 - 450 and xs.max() < 1100 + 450 and ys.min() >= 800 - 450 and ys.max() < 800 + 450
    assert np.all(r3[m].min(axis=-1) < 255) and np.all(r3[:300] == 255) and np.all(m2[:300] == 0)      # paint / padding
    # the photo away from the covered region (one pixel of margin for the down-scale) is the resized photo, untouched
    half = m[0::2, 0::2] | m[1::2, 0::2] | m[0::2, 1::2] | m[1::2, 1::2]
    grown = half.copy()
    grown[1:] |= half[:-1]; grown[:-1] |= half[1:]; grown[:, 1:] |= half[:, :-1]; grown[:, :-1] |= half[:, 1:]
    there_and_back = ru._resize_u8(ru._resize_u8(rgb, (2048, 1536), "cuda:0"), (1024, 768), "cuda:0")
    assert np.array_equal(overlap[~grown], there_and_back[~grown])
    assert (overlap[half] != there_and_back[half]).mean() > 0.5


def test_reproducible_and_capturable():
    """7: two calls give the same bits; a hipGraph capture of the call (one stream, a linear chain) replays to the same bits"""
    from chore_amd.render import rasterize_rgbad
    tri, rs = random_tri(7)
    B, Fn = tri.shape[:2]
    t = torch.from_numpy(tri).cuda()
    tex = torch.from_numpy(rs.uniform(0, 1, (B, Fn, 4, 4, 4, 3)).astype(np.float32)).cuda()
    light = torch.from_numpy(rs.uniform(0.2, 1.2, (B, Fn, 3)).astype(np.float32)).cuda()

    def call():
        return rasterize_rgbad(t, tex, light, 64, True, NEAR, FAR, TEX_EPS, (0.3, 0.2, 0.7), return_index=True)
    a, b = call(), call()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c = call()
    for _ in range(2):
        for v in c.values():
            v.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], c[k]), k
