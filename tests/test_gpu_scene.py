"""GPU: the HIP scene rasteriser (chore_scene_fwd), meshes and point clouds in one image.

Nothing here has a tolerance.  The face layer and the point layer of every expected image come from the two kernels the
scene kernel shares its passes with -- chore_render_fwd and chore_splat_fwd at ssaa = 1, where an output pixel is one sample,
so their outputs ARE the per-sample layers -- and tests/scene_ref.py composes and resolves them in numpy float32.  What is
checked is therefore the new part: which layer is in front, the blend, the ids and the resolve, bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import meshes
import scene_ref
import splat_ref
from splat_ref import FAR, NEAR

pytestmark = pytest.mark.gpu

BG = (0.25, 0.5, 0.75)
EPS = 1e-3
AMBIENT = 0.6
SENTINEL = -7.0
B, N, TS = 3, 300, 2
SHIFT = np.array([(0.0, 0.0, 0.0), (0.1, -0.05, 0.1), (-0.15, 0.1, -0.05)])      # the three images see the spheres elsewhere


@functools.lru_cache(maxsize=None)
def scene_mesh():
    """two icospheres whose vertices are [u, v, depth] as they stand, both windings: tri (3,800,3,3), textures on the 1/256
    grid (3,800,2,2,2,3), light (3,800,3) float32"""
    v1, f1 = meshes.icosphere(2, 0.5, (-0.2, 0.1, 1.5))
    v2, f2 = meshes.icosphere(1, 0.35, (0.45, -0.3, 0.8))
    v, f = np.concatenate([v1, v2]), np.concatenate([f1, f2 + len(v1)])
    f = np.concatenate([f, f[:, ::-1]])
    tri = np.stack([(v + s)[f] for s in SHIFT]).astype(np.float32)
    rs = np.random.RandomState(11)
    tex = (rs.randint(64, 256, (B, len(f), TS, TS, TS, 3)) / 256.0).astype(np.float32)
    light = rs.uniform(0.5, 1.0, (B, len(f), 3)).astype(np.float32)
    assert tri.shape == (B, 800, 3, 3)
    return tri, tex, light


@functools.lru_cache(maxsize=None)
def opacity():
    """per-face opacities in {0, 0.5, 1}"""
    return np.random.RandomState(12).choice(np.array([0.0, 0.5, 1.0], np.float32), (B, 800))


def cuda(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def parent_layers(tri, tex, light, pts, col, rad, S):
    """the per-sample layers at S x S samples from chore_render_fwd and chore_splat_fwd at ssaa = 1, rows not flipped:
    face id (B,S,S), m (B,S,S,3), zf (B,S,S), point id, p, zn"""
    from chore_amd.render import rasterize_rgbad, splat_points
    f = rasterize_rgbad(cuda(tri), cuda(tex), cuda(light), S, False, NEAR, FAR, EPS, BG, return_index=True)
    radius = cuda(rad) if np.ndim(rad) > 0 else float(rad)
    p = splat_points(cuda(pts), cuda(col), radius, S, False, NEAR, FAR, AMBIENT, BG, return_index=True)
    unflip = lambda x: x.cpu().numpy()[:, ::-1]                                     # noqa: E731
    return (f["face_index"].cpu().numpy(), unflip(f["rgb"].permute(0, 2, 3, 1)), unflip(f["depth"]),
            p["point_index"].cpu().numpy(), unflip(p["rgb"].permute(0, 2, 3, 1)), unflip(p["depth"]))


def expected(layers, op, bias, ssaa):
    """scene_ref on the layers -> dict like the kernel's outputs, plus the per-sample classes"""
    fid, m, zf, pid, p, zn = layers
    per_sample = None if op is None else np.stack([op[b][np.maximum(fid[b], 0)] for b in range(len(fid))])
    c, d, a, ident = scene_ref.compose(fid, m, zf, pid, p, zn, per_sample, bias, BG, FAR)
    rgb, depth, alpha = scene_ref.resolve(c, d, a, ssaa)
    return {"rgb": rgb, "depth": depth, "alpha": alpha, "id": ident}


def classes(layers, ident):
    fid, pid = layers[0], layers[3]
    both = (fid >= 0) & (pid >= 0)
    return {"empty": int((ident == -1).sum()), "face only": int(((fid >= 0) & (pid < 0)).sum()),
            "point only": int(((fid < 0) & (pid >= 0)).sum()), "point in front of a face": int((both & (ident < -1)).sum()),
            "face in front of a point": int((both & (ident >= 0)).sum())}


def hip_scene(tri, tex, light, pts, col, rad, size, ssaa, op=None, bias=0.0):
    from chore_amd.render import rasterize_scene
    radius = cuda(rad) if np.ndim(rad) > 0 else float(rad)
    out = rasterize_scene(cuda(tri), cuda(tex), cuda(light), cuda(pts), cuda(col), radius, cuda(op), bias, size, ssaa == 2,
                          NEAR, FAR, EPS, AMBIENT, BG, return_index=True)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["id"] = out.pop("sample_id")
    return out


def assert_same(got, want, what=""):
    for k in ("id", "rgb", "depth", "alpha"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("ssaa", [1, 2])
def test_no_visible_point_is_the_mesh_renderer(ssaa):
    """1: with a single point beyond far_z all four outputs equal rasterize_rgbad's"""
    from chore_amd.render import rasterize_rgbad
    tri, tex, light = scene_mesh()
    pts = np.tile(np.array([0.0, 0.0, FAR + 1.0], np.float32), (B, 1, 1))
    for size in (32, 33):
        got = hip_scene(tri, tex, light, pts, None, 3.0, size, ssaa)
        want = rasterize_rgbad(cuda(tri), cuda(tex), cuda(light), size, ssaa == 2, NEAR, FAR, EPS, BG, return_index=True)
        want = {k: v.cpu().numpy() for k, v in want.items()}
        want["id"] = want.pop("face_index")
        assert (want["id"] >= 0).any() and (want["id"] == -1).any()
        assert_same(got, want, size)


@pytest.mark.parametrize("ssaa", [1, 2])
def test_no_visible_face_is_the_point_renderer(ssaa):
    """2: with one back-facing triangle all four outputs equal splat_points'"""
    from chore_amd.render import rasterize_rgbad, splat_points
    tri = np.tile(np.array([[-0.9, -0.9, 1.0], [-0.9, 0.9, 1.0], [0.9, -0.9, 1.0]], np.float32), (B, 1, 1, 1))
    tex = np.ones((B, 1, TS, TS, TS, 3), np.float32)
    pts, col, rad = splat_ref.issue_cloud(5, B=B, N=N, ssaa=ssaa)
    for size in (32, 33):
        culled = rasterize_rgbad(cuda(tri), cuda(tex), None, size, ssaa == 2, NEAR, FAR, EPS, BG, return_index=True)
        assert (culled["face_index"] == -1).all()
        got = hip_scene(tri, tex, None, pts, col, rad, size, ssaa, op=np.full((B, 1), 0.5, np.float32), bias=0.25)
        want = splat_points(cuda(pts), cuda(col), cuda(rad), size, ssaa == 2, NEAR, FAR, AMBIENT, BG, return_index=True)
        want = {k: v.cpu().numpy() for k, v in want.items()}
        pim = want.pop("point_index")
        want["id"] = np.where(pim >= 0, -2 - pim, -1).astype(np.int32)
        assert (pim >= 0).any() and (pim == -1).any()
        assert_same(got, want, size)


@pytest.mark.parametrize("bias", [0.0, 0.25])
@pytest.mark.parametrize("with_opacity", [False, True])
@pytest.mark.parametrize("size", [32, 33])
def test_composite_from_the_parents_layers(size, with_opacity, bias):
    """3: at ssaa = 1 the expected image is scene_ref on chore_render_fwd's and chore_splat_fwd's outputs"""
    tri, tex, light = scene_mesh()
    pts, col, rad = splat_ref.issue_cloud(5, B=B, N=N, ssaa=1)
    op = opacity() if with_opacity else None
    layers = parent_layers(tri, tex, light, pts, col, rad, size)
    want = expected(layers, op, bias, 1)
    got = hip_scene(tri, tex, light, pts, col, rad, size, 1, op, bias)
    cls = classes(layers, want["id"])
    print("size %d opacity %s bias %g:" % (size, with_opacity, bias), cls)
    assert all(n > 20 for n in cls.values()), cls                       # every class of the rule is populated
    assert_same(got, want)
    if with_opacity:
        fid, pid = layers[0], layers[3]
        o = np.stack([op[b][np.maximum(fid[b], 0)] for b in range(B)])
        alone = (fid >= 0) & (pid < 0)
        assert sorted(np.unique(got["alpha"][:, ::-1][alone])) == [0.0, 0.5, 1.0]
        assert ((o == 0.5) & (fid >= 0) & (pid >= 0) & (want["id"] >= 0)).sum() > 20       # a blend over a point


def test_bias_moves_samples_to_the_points():
    """3b: the bias only ever turns faces in front into points in front, and does so for a good number of samples"""
    tri, tex, light = scene_mesh()
    pts, col, rad = splat_ref.issue_cloud(5, B=B, N=N, ssaa=1)
    a = hip_scene(tri, tex, light, pts, col, rad, 64, 1, None, 0.0)["id"]
    b = hip_scene(tri, tex, light, pts, col, rad, 64, 1, None, 0.25)["id"]
    moved = a != b
    assert moved.sum() > 100 and (a[moved] >= 0).all() and (b[moved] < -1).all()


@pytest.mark.parametrize("size", [32, 33, 136])
def test_ssaa2_is_the_mean_of_its_samples(size):
    """4: (size, 2) with radius r equals scene_ref on the parents' layers at (2 size, 1) with radius 2 r, resolved.  33 has
    partial 16 x 16 tiles; 136 is 272 samples and crosses the 256-sample bin boundary"""
    tri, tex, light = scene_mesh()
    pts, col, rad = splat_ref.issue_cloud(5, B=B, N=N, ssaa=2)
    op, bias = opacity(), 0.25
    layers = parent_layers(tri, tex, light, pts, col, 2 * rad, 2 * size)
    want = expected(layers, op, bias, 2)
    got = hip_scene(tri, tex, light, pts, col, rad, size, 2, op, bias)
    cls = classes(layers, want["id"])
    ident = want["id"]
    mixed = sum((ident[:, sy::2, sx::2] != ident[:, 0::2, 0::2]) for sy in (0, 1) for sx in (0, 1)) > 0
    print("size %d:" % size, cls, "output pixels with mixed winners:", int(mixed.sum()))
    assert all(n > 100 for n in cls.values()), cls
    assert mixed.sum() > 500
    assert_same(got, want)


def test_an_exact_tie_goes_to_the_face_and_a_bias_gives_it_to_the_point():
    """5: a point at a covered sample's centre with exactly the face's depth"""
    from chore_amd.render import rasterize_rgbad
    tri, tex, light = (a[:1] for a in scene_mesh())
    S = 32
    f = rasterize_rgbad(cuda(tri), cuda(tex), cuda(light), S, False, NEAR, FAR, EPS, BG, return_index=True)
    fid, zf = f["face_index"].cpu().numpy()[0], f["depth"].cpu().numpy()[0, ::-1]
    rows, cols = np.where(fid >= 0)
    k = len(rows) // 2
    j, i = int(rows[k]), int(cols[k])
    z = zf[j, i]
    assert NEAR < z < FAR
    pts = np.array([[[(2.0 * i + 1 - S) / S, (2.0 * j + 1 - S) / S, z]]], np.float32)
    col = np.array([[[1.0, 0.0, 1.0]]], np.float32)
    alone = splat_ref.splat(pts, col, 0.3, S, 1, near=NEAR, far=FAR)["index"][0]
    assert alone[j, i] == 0 and (alone >= 0).sum() == 1
    tie = hip_scene(tri, tex, light, pts, col, 0.3, S, 1, None, 0.0)
    assert tie["id"][0, j, i] == fid[j, i] and np.array_equal(tie["id"][0], fid)
    assert np.array_equal(tie["rgb"], f["rgb"].cpu().numpy())
    won = hip_scene(tri, tex, light, pts, col, 0.3, S, 1, None, 0.01)
    assert won["id"][0, j, i] == -2
    assert (won["id"][0] != fid).sum() == 1
    assert won["depth"][0, S - 1 - j, i] == z and np.array_equal(won["depth"], tie["depth"])
    assert np.array_equal(won["rgb"][0, :, S - 1 - j, i], np.array([1.0, 0.0, 1.0], np.float32))      # d2 = 0: full shade


class Call:
    """one chore_scene_fwd call with every buffer allocated up front (so that it can be recorded into a graph)"""

    def __init__(self, tri, tex, light, op, pts, col, rad, size, ssaa, bias=0.25):
        from chore_amd import _lib
        self.lib, self.h = _lib.lib, _lib.handle(0)
        self.t = {k: cuda(v) for k, v in dict(tri=tri, tex=tex, light=light, op=op, pts=pts, col=col, rad=rad).items()}
        self.B, self.F, self.N, self.size, self.ssaa, self.bias = tri.shape[0], tri.shape[1], pts.shape[1], size, ssaa, bias
        self.bg = (ctypes.c_float * 3)(*BG)
        S = size * ssaa
        nbytes = self.lib.chore_scene_workspace_bytes(self.B, self.F, self.N, size, ssaa)
        render = self.lib.chore_render_workspace_bytes(self.B, self.F, size, ssaa)
        assert nbytes == (render + 255) // 256 * 256 + self.B * S * S * 8
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.out = {"rgb": torch.full((self.B, 3, size, size), SENTINEL, device="cuda"),
                    "depth": torch.full((self.B, size, size), SENTINEL, device="cuda"),
                    "alpha": torch.full((self.B, size, size), SENTINEL, device="cuda"),
                    "id": torch.full((self.B, S, S), -9, dtype=torch.int32, device="cuda")}

    def raw(self, **over):
        """the return code of the call with some arguments replaced"""
        p = lambda x: None if x is None else x.data_ptr()     # noqa: E731
        a = {k: p(v) for k, v in self.t.items()}
        a.update({k: p(v) for k, v in self.out.items()})
        a.update(B=self.B, F=self.F, ts=TS, radius_px=0.0, N=self.N, bias=self.bias, size=self.size, ssaa=self.ssaa,
                 ambient=AMBIENT, near=NEAR, far=FAR, eps=EPS, bg=self.bg, ws=p(self.ws))
        a.update(over)
        return self.lib.chore_scene_fwd(self.h, a["tri"], a["tex"], a["light"], a["op"], a["B"], a["F"], a["ts"], a["pts"],
                                        a["col"], a["rad"], a["radius_px"], a["N"], a["bias"], a["size"], a["ssaa"],
                                        a["ambient"], a["near"], a["far"], a["eps"], a["bg"], a["rgb"], a["depth"], a["alpha"],
                                        a["id"], a["ws"], torch.cuda.current_stream().cuda_stream)

    def __call__(self):
        rc = self.raw()
        assert rc == 0, self.lib.chore_last_error(self.h)
        return self

    def numpy(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}


def test_order_independence_and_replay():
    """6: permuted points (ids mapped back), a second call and a graph replay give the same bits"""
    size, ssaa = 33, 2
    tri, tex, light = scene_mesh()
    pts, col, rad = splat_ref.issue_cloud(5, B=B, N=N, ssaa=ssaa)
    call = Call(tri, tex, light, opacity(), pts, col, rad, size, ssaa)
    a = call().numpy()
    b = call().numpy()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert (a["id"] >= 0).any() and (a["id"] < -1).any() and (a["id"] == -1).any()
    for seed in (1, 2):
        perm = np.stack([np.random.RandomState(seed * 10 + i).permutation(N) for i in range(B)])
        # twins keep their relative order so that "the smaller index" names the same point after mapping back
        for i in range(B):
            p14, p250 = np.where(perm[i] == 14)[0][0], np.where(perm[i] == 250)[0][0]
            if p14 > p250:
                perm[i][[p14, p250]] = perm[i][[p250, p14]]
        take = lambda x: np.stack([x[i][perm[i]] for i in range(B)])      # noqa: E731
        c = Call(tri, tex, light, opacity(), take(pts), take(col), take(rad), size, ssaa)().numpy()
        back = np.stack([np.where(c["id"][i] < -1, -2 - perm[i][np.maximum(-2 - c["id"][i], 0)], c["id"][i]) for i in range(B)])
        assert np.array_equal(back, a["id"])
        for k in ("rgb", "depth", "alpha"):
            assert np.array_equal(c[k], a[k]), k
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call()
    for _ in range(2):
        for v in call.out.values():
            v.fill_(-5)
        g.replay()
        c = call.numpy()
        for k in a:
            assert np.array_equal(a[k], c[k]), k


def test_disc_sizes():
    """7: discs drawn by the wave (radius above 2 samples) and one at the 64-sample clamp that overhangs a border, under the
    comparison of test 3"""
    size = 96
    tri, tex, light = scene_mesh()
    pts, col, rad = splat_ref.issue_cloud(5, B=B, N=N, ssaa=1)
    rad[:, 40:60] = np.linspace(2.5, 9.0, 20, dtype=np.float32)        # the wave path
    pts[:, 30] = (0.9, 0.2, 1.2)                                       # between the far sphere's front and the near sphere's
    rad[:, 30] = 200.0                                                 # clamped to 64 samples
    op = opacity()
    layers = parent_layers(tri, tex, light, pts, col, rad, size)
    want = expected(layers, op, 0.0, 1)
    got = hip_scene(tri, tex, light, pts, col, rad, size, 1, op, 0.0)
    assert_same(got, want)
    pid, ident = layers[3], got["id"]
    assert all((edge == 30).any() for edge in (pid[:, :, -1], pid[:, 0], pid[:, -1]))      # it overhangs three borders
    assert (pid[:, :, 0] != 30).all()                                   # and ends before the fourth
    assert (ident == -32).sum() > 200                                   # in front of the background and of the far sphere
    assert ((pid == 30) & (ident >= 0)).sum() > 50                      # and behind the near one
    assert any(((pid == n) & (ident == -2 - n)).any() for n in range(40, 60))


def test_refusals():
    """8: every bad argument returns CHORE_EINVAL before anything is launched; the size function returns 0 for the shapes"""
    tri, tex, light = scene_mesh()
    pts, col, rad = splat_ref.issue_cloud(5, B=B, N=N, ssaa=2)
    call = Call(tri, tex, light, opacity(), pts, col, rad, 32, 2)
    bad = [dict(bias=-0.5), dict(bias=float("nan")), dict(bias=-float("inf")), dict(F=0), dict(N=0), dict(B=0), dict(rgb=None),
           dict(depth=None), dict(alpha=None), dict(tri=None), dict(tex=None), dict(pts=None), dict(ws=None), dict(size=2049),
           dict(ssaa=3), dict(ts=1), dict(ambient=1.5), dict(near=2.0, far=2.0), dict(rad=None, radius_px=0.0)]
    for over in bad:
        rc = call.raw(**over)
        assert rc == -1, over
        assert b"chore_scene_fwd" in call.lib.chore_last_error(call.h), over
    out = call.numpy()
    for k in ("rgb", "depth", "alpha"):
        assert (out[k] == SENTINEL).all(), k
    assert (out["id"] == -9).all()
    size_of = call.lib.chore_scene_workspace_bytes
    assert size_of(B, 800, N, 32, 2) > 0
    for shape in ((B, 0, N, 32, 2), (B, 800, 0, 32, 2), (0, 800, N, 32, 2), (B, 800, N, 2049, 2), (B, 800, N, 4097, 1),
                  (B, 800, N, 32, 3), (B, 800, N, 0, 2)):
        assert size_of(*shape) == 0, shape
    assert call.raw(id=None) == 0                                       # the ids are optional
    assert call.raw(op=None, light=None, col=None) == 0
    torch.cuda.synchronize()


def _renderers():
    from chore_amd.render import Renderer
    from chore_amd.utils.render_utils import get_kinect_K, setup_side_renderer
    K, ratio = get_kinect_K(256)
    proj = Renderer(image_size=256, K=K, R=torch.eye(3)[None], t=torch.zeros(1, 3), orig_size=2048 * ratio)
    side = setup_side_renderer(2.0, 0., 90., image_size=192)
    return (proj, torch.tensor([0.0, 0.0, 2.0])), (side, torch.zeros(3))


def test_renderer_render_scene():
    """9: Renderer.render_scene is rasterize_scene on inputs prepared by hand, in both camera modes"""
    from chore_amd.render import face_light, rasterize_scene, vertices_to_faces, world_radius_to_pixels
    v, f = meshes.icosphere(1, 0.3)
    rs = np.random.RandomState(9)
    faces = torch.from_numpy(f.astype(np.int32))[None].cuda()
    tex = torch.from_numpy((rs.randint(64, 256, (1, len(f), 2, 2, 2, 3)) / 256.0).astype(np.float32)).cuda()
    op = torch.from_numpy(rs.choice(np.array([0.25, 0.5, 1.0], np.float32), (1, len(f)))).cuda()
    cloud = torch.from_numpy(rs.uniform(-0.45, 0.45, (1, 60, 3)).astype(np.float32)).cuda()
    col = torch.from_numpy(rs.uniform(0, 1, (1, 60, 3)).astype(np.float32)).cuda()
    for r, shift in _renderers():
        verts = torch.from_numpy(v.astype(np.float32))[None].cuda() + shift.cuda()
        pts = cloud + shift.cuda()
        assert r.fill_back
        f2 = torch.cat((faces, faces.flip(-1)), dim=1)
        t2 = torch.cat((tex, tex.permute((0, 1, 4, 3, 2, 5))), dim=1)
        light = face_light(vertices_to_faces(verts, f2), r.light_intensity_ambient, r.light_intensity_directional,
                           r.light_color_ambient, r.light_color_directional, r.light_direction)
        tri, ndc = vertices_to_faces(r.transform(verts), f2), r.transform(pts)
        focal = r.focal_pixels()
        focal = focal.cuda().view(-1, 1) if torch.is_tensor(focal) else focal
        kw = dict(image_size=r.image_size, anti_aliasing=r.anti_aliasing, near=r.near, far=r.far, eps=r.rasterizer_eps,
                  background_color=r.background_color)
        covered = {}
        for what, args, hand in (
                ("pixel radius", dict(radius=1.5), 1.5),
                ("world radius", dict(world_radius=0.02), world_radius_to_pixels(torch.tensor(0.02).cuda(), ndc[:, :, 2], focal))):
            rgb, depth, alpha = r.render_scene(verts, faces, tex, pts, col, face_opacity=op, point_depth_bias=0.05, **args)
            want = rasterize_scene(tri, t2, light, ndc, col, hand, torch.cat((op, op), dim=1), 0.05, **kw)
            assert torch.equal(rgb, want["rgb"]) and torch.equal(depth, want["depth"]) and torch.equal(alpha, want["alpha"]), what
            assert rgb.shape == (1, 3, r.image_size, r.image_size)
            vals = set(np.unique(alpha.cpu().numpy()).tolist())
            assert {0.0, 1.0} <= vals and vals & {0.25, 0.5}, (what, sorted(vals)[:8])    # background, points, translucent faces
            points_only = r.render_points(pts, col, **args)[2]
            covered[what] = float((points_only > 0).sum())
        assert covered["world radius"] != covered["pixel radius"]
        # F == 0: the point path; N == 0: the mesh path
        none = r.render_scene(verts, faces[:, :0], tex[:, :0], pts, col, radius=2.5)
        for a, b in zip(none, r.render_points(pts, col, radius=2.5)):
            assert torch.equal(a, b)
        none = r.render_scene(verts, faces, tex, pts[:, :0], None)
        for a, b in zip(none, r.render(verts, faces, tex)):
            assert torch.equal(a, b)
    with pytest.raises(ValueError):
        rasterize_scene(tri, t2, light, ndc, col, 2.5, point_depth_bias=-1.0)
    with pytest.raises(RuntimeError):
        rasterize_scene(tri.cpu(), t2, light, ndc, col, 2.5)


def test_rasterize_scene_fallback_ids():
    """9b: rasterize_scene without faces / without points returns the ids in the scene's convention"""
    from chore_amd.render import rasterize_rgbad, rasterize_scene, splat_points
    tri, tex, light = (cuda(a) for a in scene_mesh())
    pts, col, rad = (cuda(a) for a in splat_ref.issue_cloud(5, B=B, N=N, ssaa=2))
    a = rasterize_scene(tri[:, :0], tex[:, :0], None, pts, col, rad, image_size=32, return_index=True)
    b = splat_points(pts, col, rad, 32, return_index=True)
    assert torch.equal(a["sample_id"], torch.where(b["point_index"] >= 0, -2 - b["point_index"], b["point_index"]))
    assert torch.equal(a["rgb"], b["rgb"]) and "point_index" not in a
    a = rasterize_scene(tri, tex, light, pts[:, :0], image_size=32, return_index=True)
    b = rasterize_rgbad(tri, tex, light, 32, return_index=True)
    assert torch.equal(a["sample_id"], b["face_index"]) and torch.equal(a["rgb"], b["rgb"]) and "face_index" not in a
    # an opacity is honoured without points too: over the background, alpha = the opacity
    half = rasterize_scene(tri, tex, light, pts[:, :0], face_opacity=torch.full((B, 800), 0.5).cuda(), image_size=32,
                           anti_aliasing=False, background_color=BG, return_index=True)
    assert torch.equal(half["sample_id"], rasterize_rgbad(tri, tex, light, 32, False, return_index=True)["face_index"])
    assert sorted(np.unique(half["alpha"].cpu().numpy())) == [0.0, 0.5]
