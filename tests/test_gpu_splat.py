"""GPU: the HIP point rasteriser (chore_splat_fwd) through the C ABI against the numpy restatements of tests/splat_ref.py
(float32 for the winners, float64 for the values), and chore_amd.render.splat_points / Renderer.render_points on top."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import splat_ref
from splat_ref import FAR, NEAR

pytestmark = pytest.mark.gpu

BG = (0.25, 0.5, 0.75)
SENTINEL = -7.0


class Call:
    """one chore_splat_fwd call with every buffer allocated up front (so that it can be recorded into a graph)"""

    def __init__(self, pts, colors, radius, size, ssaa, ambient=0.6, near=NEAR, far=FAR, background=BG, index=True):
        from chore_amd import _lib
        self.lib, self.h = _lib.lib, _lib.handle(0)
        t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float32)).cuda().contiguous()     # noqa: E731
        self.pts, self.col = t(pts), t(colors)
        self.rad = t(radius) if np.ndim(radius) > 0 else None
        self.radius_px = 0.0 if self.rad is not None else float(radius)
        self.B, self.N = self.pts.shape[:2]
        self.size, self.ssaa, self.ambient, self.near, self.far = size, ssaa, ambient, near, far
        self.bg = (ctypes.c_float * 3)(*background)
        S = size * ssaa
        nbytes = self.lib.chore_splat_workspace_bytes(self.B, self.N, size, ssaa)
        assert nbytes == self.B * S * S * 8
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.out = {"rgb": torch.full((self.B, 3, size, size), SENTINEL, device="cuda"),
                    "depth": torch.full((self.B, size, size), SENTINEL, device="cuda"),
                    "alpha": torch.full((self.B, size, size), SENTINEL, device="cuda")}
        if index:
            self.out["index"] = torch.full((self.B, S, S), -9, dtype=torch.int32, device="cuda")

    def raw(self, **over):
        """the return code of the call with some arguments replaced"""
        p = lambda x: None if x is None else x.data_ptr()     # noqa: E731
        a = dict(pts=p(self.pts), col=p(self.col), rad=p(self.rad), radius_px=self.radius_px, B=self.B, N=self.N,
                 size=self.size, ssaa=self.ssaa, ambient=self.ambient, near=self.near, far=self.far, bg=self.bg,
                 rgb=p(self.out["rgb"]), depth=p(self.out["depth"]), alpha=p(self.out["alpha"]), index=p(self.out.get("index")),
                 ws=p(self.ws))
        a.update(over)
        return self.lib.chore_splat_fwd(self.h, a["pts"], a["col"], a["rad"], a["radius_px"], a["B"], a["N"], a["size"], a["ssaa"],
                                        a["ambient"], a["near"], a["far"], a["bg"], a["rgb"], a["depth"], a["alpha"], a["index"],
                                        a["ws"], torch.cuda.current_stream().cuda_stream)

    def __call__(self):
        rc = self.raw()
        assert rc == 0, self.lib.chore_last_error(self.h)
        return self

    def numpy(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}


def hip_splat(pts, colors, radius, size, ssaa, **kw):
    return Call(pts, colors, radius, size, ssaa, **kw)().numpy()


SCALAR_RADIUS = 1.7       # output pixels, for the calls without per-point radii


@functools.lru_cache(maxsize=None)
def case(size, ssaa, per_point, ambient=0.6, exact=False):
    """the cloud of the winner tests at one grid with both restatements (computed once, never modified).  exact: depths on
    the 1/64 grid (the colours are on the 1/256 grid already), so that sums of four are exact in float32"""
    pts, col, rad = splat_ref.issue_cloud(0, ssaa=ssaa)
    if exact:
        z = pts[..., 2]
        pts[..., 2] = np.where(np.isfinite(z), np.round(z * 64) / 64, z).astype(np.float32)
    radius = rad if per_point else SCALAR_RADIUS
    kw = dict(ambient=ambient, near=NEAR, far=FAR, background=BG)
    r32 = splat_ref.splat(pts, col, radius, size, ssaa, dtype=np.float32, **kw)
    r64 = splat_ref.splat(pts, col, radius, size, ssaa, dtype=np.float64, **kw)
    return pts, col, radius, r32, r64


GRID_CASES = [(size, ssaa, pp) for size, ssaa in splat_ref.ISSUE_GRIDS for pp in (True, False)]


@pytest.mark.parametrize("size,ssaa,per_point", GRID_CASES)
def test_winners_exact(size, ssaa, per_point):
    """1: sample_point_index equals the float32 restatement on every sample of every image"""
    pts, col, radius, r32, _ = case(size, ssaa, per_point)
    out = hip_splat(pts, col, radius, size, ssaa)
    idx = out["index"]
    assert idx.shape == (3, size * ssaa, size * ssaa)
    cover = (r32["index"] >= 0).mean(axis=(1, 2))
    assert (cover > 0.3).all() and (cover < 0.995).all(), cover          # some samples stay empty in every image
    assert np.array_equal(idx, r32["index"])
    present = set(np.unique(idx))
    skipped = {0, 1, 2, 3, 8, 9, 10} | ({11, 12, 13} if per_point else set())
    assert not present & skipped                      # outside the frame / the depth range, NaN, radius <= 0
    assert 14 in present and 250 not in present       # identical twins: the smaller index
    assert not np.array_equal(idx[0], idx[1])
    if per_point:
        assert {4, 5, 6, 7} <= present                # a disc straddling each of the four borders
        assert 20 in present and 21 not in present    # hidden behind a larger, nearer disc


def _errors(out, ref, ok):
    """max |out - ref| of rgb, depth, alpha over the pixels `ok` (B,size,size)"""
    e = {}
    for k in ("rgb", "depth", "alpha"):
        d = np.abs(out[k].astype(np.float64) - ref[k].astype(np.float64))
        m = np.broadcast_to(ok[:, None], d.shape) if k == "rgb" else ok
        e[k] = float(d[m].max())
    return e


@pytest.mark.parametrize("size,ssaa,per_point", GRID_CASES)
@pytest.mark.parametrize("ambient", [0.6, 1.0])
def test_values_against_float64(size, ssaa, per_point, ambient):
    """2: rgb / depth / alpha against the float64 restatement within 4 x E32, E32 = max |restatement32 - restatement64| over
    the pixels whose winners agree; equality where E32 == 0, which ambient = 1 with colours and depths on a dyadic grid
    guarantees (the shade is exactly 1 and every mean is an exact float32 sum).  Empty pixels hold the background exactly."""
    exact = ambient == 1.0
    pts, col, radius, r32, r64 = case(size, ssaa, per_point, ambient, exact)
    out = hip_splat(pts, col, radius, size, ssaa, ambient=ambient)
    covered = (r32["index"] >= 0).sum()
    agree = splat_ref.pixels_agree(r32["index"], r64["index"], ssaa)
    assert (r32["index"] != r64["index"]).sum() <= 0.005 * covered
    assert np.array_equal(out["index"], r32["index"])
    e32 = _errors(r32, r64, agree)
    err = _errors(out, r64, agree)
    print("size %d ssaa %d per_point %s ambient %g: E32 %s kernel %s" % (size, ssaa, per_point, ambient, e32, err))
    for k in e32:
        if exact:
            assert e32[k] == 0.0, (k, e32[k])
        if e32[k] == 0.0:
            assert np.array_equal(out[k][np.broadcast_to(agree[:, None], out[k].shape) if k == "rgb" else agree],
                                  r64[k][np.broadcast_to(agree[:, None], out[k].shape) if k == "rgb" else agree]), k
        else:
            assert err[k] <= 4 * e32[k], (k, err[k], e32[k])
    empty = splat_ref.pixels_agree(r32["index"], np.full_like(r32["index"], -1), ssaa)
    assert empty.any()
    for c in range(3):
        assert (out["rgb"][:, c][empty] == np.float32(BG[c])).all()
    assert (out["depth"][empty] == np.float32(FAR)).all() and (out["alpha"][empty] == 0).all()


def test_order_independence_and_replay():
    """3: seeded permutations of the cloud (indices mapped back), a second call and a graph replay are bit-equal"""
    size, ssaa = 33, 2
    pts, col, rad, _, _ = case(size, ssaa, True)
    call = Call(pts, col, rad, size, ssaa)
    a = call().numpy()
    b = call().numpy()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for seed in (1, 2):
        perm = np.stack([np.random.RandomState(seed * 10 + i).permutation(pts.shape[1]) for i in range(pts.shape[0])])
        take = lambda x: np.stack([x[i][perm[i]] for i in range(len(perm))])      # noqa: E731
        # twins keep their relative order so that "the smaller index" names the same point after mapping back
        for i in range(len(perm)):
            p14, p250 = np.where(perm[i] == 14)[0][0], np.where(perm[i] == 250)[0][0]
            if p14 > p250:
                perm[i][[p14, p250]] = perm[i][[p250, p14]]
        c = hip_splat(take(pts), take(col), take(rad), size, ssaa)
        back = np.stack([np.where(c["index"][i] >= 0, perm[i][np.maximum(c["index"][i], 0)], -1) for i in range(len(perm))])
        assert np.array_equal(back, a["index"])
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


def test_same_grid_as_the_meshes():
    """4: a point at the normalised centre of sample (i, j) with radius 0.3 sample wins exactly that sample; a small triangle
    around the same position covers it in the mesh rasteriser's face_index; v > 0 is the upper half of the image"""
    from chore_amd.render import rasterize_rgbad
    size, ssaa = 32, 2
    S = size * ssaa
    rs = np.random.RandomState(4)
    ij = rs.randint(0, S, (20, 2))
    centre = lambda i: np.float32((2.0 * i + 1 - S) / S)     # noqa: E731  raster_common.h raster_centre
    pts = np.array([[[centre(i), centre(j), 1.0]] for i, j in ij], np.float32)               # 20 images of one point
    out = hip_splat(pts, None, 0.3 / ssaa, size, ssaa, ambient=1.0)
    d = np.float32(1.2 / S)
    tri = np.array([[[[u - d, v - d, 1.0], [u + d, v - d, 1.0], [u, v + d, 1.0]]] for (u, v, _), in pts], np.float32)
    tri = np.concatenate([tri, tri[:, :, ::-1]], 1)
    tex = torch.ones(20, 2, 2, 2, 2, 3, device="cuda")
    fim = rasterize_rgbad(torch.from_numpy(np.ascontiguousarray(tri)).cuda(), tex, None, size, True, NEAR, FAR,
                          return_index=True)["face_index"].cpu().numpy()
    for k, (i, j) in enumerate(ij):
        want = np.full((S, S), -1, np.int32)
        want[j, i] = 0
        assert np.array_equal(out["index"][k], want), (k, i, j)
        assert fim[k, j, i] >= 0, (k, i, j)
    up = hip_splat(np.array([[[0.1, 0.5, 1.0]]], np.float32), None, 2.0, size, ssaa)
    rows = np.where(up["alpha"][0].sum(axis=1) > 0)[0]
    assert len(rows) and rows.max() < size // 2


def test_single_point():
    """5a: N = 1"""
    pts = np.array([[[0.0, 0.0, 1.5]]], np.float32)
    col = np.array([[[0.5, 0.25, 1.0]]], np.float32)
    out = hip_splat(pts, col, 3.0, 16, 2)
    ref = splat_ref.splat(pts, col, 3.0, 16, 2, near=NEAR, far=FAR, background=BG)
    assert np.array_equal(out["index"], ref["index"]) and (out["index"] == 0).sum() > 20
    assert np.array_equal(out["alpha"], ref["alpha"])


def test_many_points_many_workgroups():
    """5b: N = 70 001 at size 64 (indices above 16 bits, 1 094 one-wave workgroups): the winners on a seeded 4 096-sample subset and the
    coverage count against the float32 restatement"""
    N, size, ssaa = 70001, 64, 2
    S = size * ssaa
    rs = np.random.RandomState(5)
    pts = np.concatenate([rs.uniform(-1.05, 1.05, (1, N, 2)), rs.uniform(0.5, 3.0, (1, N, 1))], -1).astype(np.float32)
    rad = (rs.uniform(0.3, 0.6, (1, N)) / ssaa).astype(np.float32)     # small: some samples stay empty
    rad[0, 65536:65600] = 3.0 / ssaa
    pts[0, 65536:65600, 2] = 0.2              # points with indices past 2^16 that win their samples
    out = hip_splat(pts, None, rad, size, ssaa, ambient=1.0)
    ref = splat_ref.splat(pts, None, rad, size, ssaa, ambient=1.0, near=NEAR, far=FAR, background=BG)
    sub = rs.choice(S * S, 4096, replace=False)
    got, want = out["index"].reshape(-1)[sub], ref["index"].reshape(-1)[sub]
    assert np.array_equal(got, want)
    assert (want > 65535).any() and (want == -1).any()
    assert (out["index"] >= 0).sum() == (ref["index"] >= 0).sum()


def test_radius_clamp_overhangs_every_border():
    """5c: radius 200 px equals radius 32 px (both 64 samples after the clamp) bit for bit, the disc overhanging all borders"""
    size, ssaa = 48, 2
    pts = np.array([[[0.05, -0.1, 1.0], [0.6, 0.6, 0.5]]], np.float32)
    col = np.array([[[1.0, 0.5, 0.25], [0.0, 1.0, 0.0]]], np.float32)
    a = hip_splat(pts, col, np.array([[200.0, 1.0]], np.float32), size, ssaa)
    b = hip_splat(pts, col, np.array([[32.0, 1.0]], np.float32), size, ssaa)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    idx = a["index"][0]
    assert (idx[0] == 0).any() and (idx[-1] == 0).any() and (idx[:, 0] == 0).any() and (idx[:, -1] == 0).any()
    assert (idx == -1).any() and (idx == 1).any()          # the corners stay empty; the small near point wins its disc
    ref = splat_ref.splat(pts, col, np.array([[200.0, 1.0]], np.float32), size, ssaa, near=NEAR, far=FAR, background=BG)
    assert np.array_equal(idx, ref["index"][0])


def test_refusals():
    """6: every bad argument returns CHORE_EINVAL, chore_last_error names the function, and no output is touched"""
    pts, col, rad, _, _ = case(32, 2, True)
    call = Call(pts, col, rad, 32, 2)
    bad = [dict(pts=None), dict(rgb=None), dict(depth=None), dict(alpha=None), dict(N=0), dict(B=0), dict(ssaa=3), dict(ssaa=0),
           dict(size=2049), dict(ambient=-0.1), dict(ambient=1.5), dict(near=2.0, far=2.0), dict(near=3.0, far=1.0),
           dict(rad=None, radius_px=0.0), dict(rad=None, radius_px=-1.0)]
    for over in bad:
        rc = call.raw(**over)
        assert rc == -1, over
        assert b"chore_splat_fwd" in call.lib.chore_last_error(call.h), over
    out = call.numpy()
    for k in ("rgb", "depth", "alpha"):
        assert (out[k] == SENTINEL).all(), k
    assert (out["index"] == -9).all()
    assert call.lib.chore_splat_workspace_bytes(1, 10, 2049, 2) == 0


def _covered(alpha):
    return float((alpha > 0).sum())


def test_render_points_world_radius_and_modes():
    """7: a world radius halves the square root of the covered sample count (+-1) from z to 2z; both camera modes agree with
    splat_points fed by Renderer.transform.  render_points has no ambient argument (the shade is splat_points' default, 0.6,
    not the 1 the single-point check was specified with): the check counts alpha > 0, which the shade does not enter."""
    from chore_amd.render import Renderer, splat_points
    from chore_amd.utils.render_utils import get_kinect_K, setup_side_renderer
    K, ratio = get_kinect_K(512)
    proj = Renderer(image_size=512, K=K, R=torch.eye(3)[None], t=torch.zeros(1, 3), orig_size=2048 * ratio, anti_aliasing=False)
    side = setup_side_renderer(2.0, 0., 90., image_size=256)
    side.anti_aliasing = False
    for r in (proj, side):
        roots = []
        for k in (1.0, 2.0):
            if r is proj:
                p = torch.tensor([[[0.0, 0.0, 1.5 * k]]], device="cuda")
            else:       # on the viewing axis of the look_at camera at distances d and 2d from the eye
                eye = torch.tensor(r.eye, dtype=torch.float32)
                p = (eye * (1 - 0.45 * k))[None, None].cuda()
            _, _, alpha = r.render_points(p, world_radius=0.06)
            roots.append(np.sqrt(_covered(alpha)))
        assert roots[0] > 8 and abs(roots[0] / 2 - roots[1]) <= 1.0, roots
    rs = np.random.RandomState(7)
    cloud = torch.from_numpy(rs.uniform(-0.4, 0.4, (2, 200, 3)).astype(np.float32)).cuda()
    col = torch.from_numpy(rs.uniform(0, 1, (2, 200, 3)).astype(np.float32)).cuda()
    for r, shift in ((proj, torch.tensor([0.0, 0.0, 2.0])), (side, torch.zeros(3))):
        p = cloud + shift.cuda()
        rgb, depth, alpha = r.render_points(p, col, radius=2.5)
        want = splat_points(r.transform(p), col, 2.5, r.image_size, r.anti_aliasing, r.near, r.far,
                            background_color=r.background_color)
        assert torch.equal(rgb, want["rgb"]) and torch.equal(depth, want["depth"]) and torch.equal(alpha, want["alpha"])
        assert 0.005 < (alpha > 0).float().mean() < 0.9
    empty = splat_points(torch.zeros(2, 0, 3, device="cuda"), image_size=8, background_color=BG, return_index=True)
    assert empty["rgb"].shape == (2, 3, 8, 8) and torch.equal(empty["rgb"][0, :, 0, 0].cpu(), torch.tensor(BG))
    assert (empty["depth"] == 100).all() and (empty["alpha"] == 0).all() and (empty["point_index"] == -1).all()
    with pytest.raises(RuntimeError):
        splat_points(torch.zeros(1, 4, 3))
