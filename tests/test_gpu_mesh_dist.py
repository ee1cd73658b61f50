"""GPU: the point-to-mesh distance kernel (chore_mesh_dist_fwd), chore_amd.preprocess.mesh_distance and BoundarySampler
against the float64 restatement of the contract in tests/mesh_dist_ref.py and known answers.

The bound of every distance comparison is 8 x E32, E32 = the largest |float32 - float64| of the restatement itself on a
seeded subsample (>= 2 000 points, every sigma and grid points) of the scene's query points against the same mesh, computed
here on every run (the `scene` fixture; the box has its own).  Tests whose inputs are too few to measure an E32 of their own
(single triangles, N = 1 ... 4 097 on small spheres) use the body blob's: their coordinates lie in the same binades.
Measured on an MI355X: see DESIGN.md, 'Mesh distance'."""
import os

import numpy as np
import pytest
import torch

import mesh_dist_ref as ref
from conftest import GOLDEN
from meshes import icosphere

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(GOLDEN, "assets")
CLOSEST_EXTRA = 4.2e-7        # sqrt(3) x half an ulp of the [4, 8) binade: rounding of a float32 point inside get_bounds()


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def body_mesh():
    from chore_amd.utils.synth import uv_ellipsoid
    v, f = uv_ellipsoid(center=(0.1, 0.2, 2.2))
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    return f32(v), f


def obj_mesh():
    v, f = icosphere(3, 0.35, (0.45, 0.1, 2.3))
    assert f.shape == (1280, 3)
    return f32(v), f


BOX = ((-0.3, -0.2, 2.0), (0.4, 0.5, 2.6))


def box_mesh():
    v, f = ref.box_mesh(BOX[0], BOX[1], 12)
    return f32(v), f


def gpu_dist(P, V, F, want=("dist", "face_idx", "closest", "vert_idx")):
    from chore_amd.preprocess import mesh_distance
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt))).cuda()      # noqa: E731
    out = mesh_distance(t(P, np.float32), t(V, np.float32), t(F, np.int32), want)
    return {k: v.cpu().numpy() for k, v in zip(want, out)}


def e32_of(P, V, F, tag=None, n=2400, seed=77):
    """E32 on a seeded subsample of >= 2 000 of the points (all of them if there are fewer than n)"""
    sel = np.random.RandomState(seed).permutation(len(P))[:n]
    if tag is not None:
        assert len(sel) >= 2000 and set(np.unique(tag[sel])) == {-1, 0, 1, 2}
    d64 = ref.mesh_distance_pruned(P[sel], V, F, np.float64)[0]
    d32 = ref.mesh_distance_pruned(P[sel], V, F, np.float32)[0]
    return float(np.abs(d32.astype(np.float64) - d64).max())


@pytest.fixture(scope="module")
def scene():
    body, obj = body_mesh(), obj_mesh()
    P, tag = ref.sampler_points([body, obj], 1700, 100, np.random.RandomState(0))
    E32 = {k: e32_of(P, *m, tag) for k, m in (("body", body), ("obj", obj))}
    return dict(body=body, obj=obj, P=P, tag=tag, E32=E32)


def check_outputs(P, V, F, out, D64, E32, what):
    """6 and 7 for one mesh: every point, no exclusions"""
    bound = 8 * E32
    dist = out["dist"].astype(np.float64)
    err = np.abs(dist - D64).max()
    print("%s: E32 %.3e  bound %.3e  kernel max |dist - D64| %.3e (%.2f E32)" % (what, E32, bound, err, err / E32))
    assert np.isfinite(out["dist"]).all() and err <= bound, (what, err, bound)
    if "face_idx" in out:
        fi = out["face_idx"]
        assert fi.min() >= 0 and fi.max() < len(F)
        d_face, _ = ref.point_to_face(P, V, F, fi)
        print("%s: max (dist to face_idx - D64) %.3e" % (what, (d_face - D64).max()))
        assert (d_face <= D64 + bound).all()
        if "closest" in out:
            C = out["closest"].astype(np.float64)
            d_c, _ = ref.point_to_face(C, V, F, fi)
            gap = np.abs(np.linalg.norm(P - C, axis=1) - dist).max()
            print("%s: closest off its face by <= %.3e, | |p - closest| - dist | <= %.3e" % (what, d_c.max(), gap))
            assert d_c.max() <= bound + CLOSEST_EXTRA and gap <= bound + CLOSEST_EXTRA
    if "vert_idx" in out:
        vi = out["vert_idx"]
        assert vi.min() >= 0 and vi.max() < len(V)
        dv, _ = ref.nearest_vertex(P, V)
        got = np.linalg.norm(P - V[vi], axis=1)
        print("%s: max |p - V[vert_idx]| / nearest - 1 = %.3e" % (what, (got / np.maximum(dv, 1e-300) - 1).max()))
        assert (got <= (1 + 1e-6) * dv).all()


def test_distances_and_indices(scene):
    """6, 7: body blob and icosphere, surface samples + sigma N(0,1) at the three sigmas and grid points"""
    P = scene["P"]
    for name in ("body", "obj"):
        V, F = scene[name]
        D64 = ref.mesh_distance_pruned(P, V, F)[0]
        check_outputs(P, V, F, gpu_dist(P, V, F), D64, scene["E32"][name], name)


def test_known_box(scene):
    """8: the triangulated box against the closed form, inside and outside points"""
    V, F = box_mesh()
    rs = np.random.RandomState(1)
    P = f32(rs.rand(2400, 3) * 1.6 + np.array([-0.8, -0.7, 1.5]))
    E32 = e32_of(P, V, F)
    lo, hi = f32(BOX[0]), f32(BOX[1])
    inside = ((P > lo) & (P < hi)).all(1)
    assert inside.sum() > 100 and (~inside).sum() > 1000
    check_outputs(P, V, F, gpu_dist(P, V, F), ref.box_distance(P, lo, hi), E32, "box")


def test_known_points_on_the_mesh(scene):
    """8: points on a vertex, on an edge, on a face are at distance 0 within the bound"""
    V, F = scene["body"]
    E32 = scene["E32"]["body"]
    rs = np.random.RandomState(5)
    fs = rs.choice(len(F), 300, replace=False)
    t = V[F[fs]]
    w = rs.dirichlet((1, 1, 1), 300)
    P = f32(np.concatenate([V[rs.choice(len(V), 300, replace=False)], 0.5 * (t[:, 0] + t[:, 1]), 0.25 * t[:, 1] + 0.75 * t[:, 2],
                            (t * w[:, :, None]).sum(1)]))
    out = gpu_dist(P, V, F)
    D64 = ref.mesh_distance_pruned(P, V, F)[0]
    assert D64.max() <= CLOSEST_EXTRA                       # only the rounding of the constructed points to float32
    print("on the mesh: max dist %.3e (vertices %.3e)" % (out["dist"].max(), out["dist"][:300].max()))
    check_outputs(P, V, F, out, D64, E32, "on the mesh")


def test_known_degenerate_triangles(scene):
    """8: zero-area triangles are the segment or the point they degenerate to; finite results"""
    E32 = scene["E32"]["body"]
    V = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 2, 0]], np.float64)
    rs = np.random.RandomState(6)
    P = f32(np.concatenate([[[0.5, 1, 0], [3, 0, 1], [-1, -1, 0], [1.0, 1.0, 0.5], [0, 0, 0], [1, 0, 0], [0, 1, 0]],
                            rs.uniform(-2, 3, (200, 3))]))

    def seg(p, a, b):
        t = np.clip(((p - a) @ (b - a)) / max((b - a) @ (b - a), 1e-300), 0, 1)
        return np.linalg.norm(p - (a + t[:, None] * (b - a)), axis=1)
    cases = [([0, 1, 2], seg(P, V[0], V[2])), ([0, 2, 1], seg(P, V[0], V[2])), ([1, 0, 2], seg(P, V[0], V[2])),
             ([0, 0, 3], seg(P, V[0], V[3])), ([0, 3, 3], seg(P, V[0], V[3])), ([3, 0, 0], seg(P, V[0], V[3])),
             ([1, 1, 1], np.linalg.norm(P - V[1], axis=1))]
    for f, want in cases:
        out = gpu_dist(P, V, np.array([f]))
        assert all(np.isfinite(v).all() for v in out.values()), f
        err = np.abs(out["dist"] - want).max()
        print(f, "max error %.3e" % err)
        assert err <= 8 * E32, (f, err)
        assert np.all(out["face_idx"] == 0)
        assert np.abs(np.linalg.norm(P - out["closest"], axis=1) - want).max() <= 8 * E32 + CLOSEST_EXTRA
    # all of them in one mesh, with a proper triangle: the minimum over the faces
    F = np.array([c[0] for c in cases] + [[0, 1, 3]])
    out = gpu_dist(P, V, F)
    assert np.abs(out["dist"] - ref.mesh_distance_brute(P, V, F)[0]).max() <= 8 * E32


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_shapes_batched(scene, N):
    """9: B = 3 with different vertex sets, N not a multiple of anything"""
    from chore_amd.preprocess import mesh_distance
    v0, F = icosphere(2, 0.3, (0.2, 0.1, 2.2))
    Vs = f32(np.stack([v0, v0 * np.array([1.0, 2.0, 0.7]) + 0.05, v0[::-1] * 1.3 - 0.4]))
    rs = np.random.RandomState(N)
    P = f32(np.stack([ref.surface_samples(Vs[b], F, N, rs) + 0.02 * rs.standard_normal((N, 3)) for b in range(3)]))
    E32 = scene["E32"]["body"]
    names = ("dist", "face_idx", "closest", "vert_idx")
    out = mesh_distance(torch.from_numpy(P).float().cuda(), torch.from_numpy(Vs).float().cuda(), torch.from_numpy(F).cuda(), names)
    assert [tuple(o.shape) for o in out] == [(3, N), (3, N), (3, N, 3), (3, N)]
    assert [o.dtype for o in out] == [torch.float32, torch.int32, torch.float32, torch.int32]
    for b in range(3):
        ob = {k: o[b].cpu().numpy() for k, o in zip(names, out)}
        check_outputs(P[b], Vs[b], F, ob, ref.mesh_distance_brute(P[b], Vs[b], F)[0], E32, "B=3 N=%d image %d" % (N, b))


def test_shapes_one_face(scene):
    """9: F = 1, V = 3"""
    V = f32([[0.1, 0.2, 2.0], [0.9, 0.1, 2.2], [0.3, 0.8, 2.5]])
    F = np.array([[0, 1, 2]])
    P = f32(np.random.RandomState(8).uniform(-1, 3, (777, 3)))
    E32 = scene["E32"]["body"]
    check_outputs(P, V, F, gpu_dist(P, V, F), ref.mesh_distance_brute(P, V, F)[0], E32, "F=1")


def test_full_frame_and_optional_outputs(scene):
    """9: (1, 110 090, 6 890, 13 776): a seeded 20 000-point subsample against the pruned restatement, isfinite on all;
    the optional outputs in every combination leave the bits of dist (and of each other) unchanged"""
    V, F = scene["body"]
    P, tag = ref.sampler_points([scene["body"], scene["obj"]], 36330, 367, np.random.RandomState(9))
    P = P[:110090]
    assert P.shape == (110090, 3)
    full = gpu_dist(P, V, F)
    assert all(np.isfinite(v).all() for v in full.values())
    sel = np.random.RandomState(10).permutation(len(P))[:20000]
    E32 = scene["E32"]["body"]
    sub = {k: v[sel] for k, v in full.items()}
    check_outputs(P[sel], V, F, sub, ref.mesh_distance_pruned(P[sel], V, F)[0], E32, "full frame")
    opt = ("face_idx", "closest", "vert_idx")
    for mask in range(7):
        want = ("dist",) + tuple(n for k, n in enumerate(opt) if mask >> k & 1)
        got = gpu_dist(P, V, F, want)
        for k in want:
            assert np.array_equal(got[k], full[k]), (want, k)


def test_cpu_tensors_are_refused():
    from chore_amd.preprocess import mesh_distance
    with pytest.raises(RuntimeError):
        mesh_distance(torch.zeros(4, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))


def test_reproducible_and_capturable(scene):
    """10: two eager calls and a hipGraph replay give the same bits"""
    from chore_amd.preprocess import mesh_distance
    V, F = scene["body"]
    p = torch.from_numpy(scene["P"]).float().cuda()
    v, f = torch.from_numpy(V).float().cuda(), torch.from_numpy(F).int().cuda()
    names = ("dist", "face_idx", "closest", "vert_idx")

    def call():
        return mesh_distance(p, v, f, names)
    a, b = call(), call()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
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
        for t in c:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k, x, y in zip(names, a, c):
            assert torch.equal(x, y), k


def test_surface_sampling(scene):
    """11: samples lie on the face they were drawn on; triangle choice is area-weighted; grid points are inside the bounds"""
    from chore_amd.preprocess.boundary_sampler import BoundarySampler, sample_surface
    V, F = scene["body"]
    E32 = scene["E32"]["body"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    pts, face = sample_surface(torch.from_numpy(V).float().cuda(), torch.from_numpy(F).cuda(), 20000, gen)
    assert pts.shape == (20000, 3) and pts.dtype == torch.float32 and face.shape == (20000,)
    d, _ = ref.point_to_face(pts.cpu().numpy().astype(np.float64), V, F, face.cpu().numpy())
    print("surface samples off their face by <= %.3e" % d.max())
    assert d.max() <= 8 * E32 + CLOSEST_EXTRA
    assert len(np.unique(face.cpu().numpy())) > 5000
    # areas 1 : 3
    V2 = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 1], [3, 0, 1], [0, 2, 1]], dtype=torch.float32).cuda()
    F2 = torch.tensor([[0, 1, 2], [3, 4, 5]]).cuda()
    n = 100000
    _, face2 = sample_surface(V2, F2, n, gen)
    small = int((face2 == 0).sum())
    print("small triangle drawn %d times of %d" % (small, n))
    assert abs(small - 25000) <= 685
    # batched form: every image samples its own vertices
    Vb = torch.stack([V2, V2 + 5.0])
    pb, fb = sample_surface(Vb, F2, 1000, gen)
    assert pb.shape == (2, 1000, 3) and fb.shape == (2, 1000) and pb[0].max() <= 3.0 and pb[1].min() >= 5.0
    s = BoundarySampler(part_labels=np.zeros(6890, np.int32), seed=1)
    bmin, bmax = BoundarySampler.get_bounds()
    g = s.get_grid_samples(bmin, bmax, 50000)
    assert g.shape == (50000, 3) and g.dtype == np.float64 and (g >= bmin).all() and (g <= bmax).all()
    assert np.abs(g.mean(0) - (bmin + bmax) / 2).max() < 0.05 and (g.max(0) - g.min(0) > 0.99 * (bmax - bmin)).all()


class _Mesh:
    def __init__(self, v, f):
        self.v, self.f = v, f


def _parts_ok(P, V, labels, parts):
    """rule of 7 through the label table: parts[i] is the label of a vertex no farther than (1 + 1e-6) x the nearest one"""
    from scipy.spatial import cKDTree
    d, i = cKDTree(V).query(P, k=4)
    ok = (labels[i] == np.asarray(parts)[:, None]) & (d <= (1 + 1e-6) * d[:, :1])
    return ok.any(1)


def test_boundary_sample_all(scene):
    """12: the dictionary of one frame at the default recipe, re-labelled with the restatement, every point"""
    from chore_amd.lib_smpl.body_landmark import BodyLandmarks
    from chore_amd.preprocess.boundary_sampler import BoundarySampler
    from chore_amd.recon.assets import FileAssets
    labels = FileAssets(ASSETS).part_labels()
    lm = BodyLandmarks(ASSETS)
    (Vh, Fh), (Vo, Fo) = scene["body"], scene["obj"]
    smpl, obj = _Mesh(Vh, Fh), _Mesh(Vo, Fo)
    sigmas, ratios = [0.08, 0.02, 0.003], [0.01, 0.49, 0.5]
    E32h, E32o = scene["E32"]["body"], scene["E32"]["obj"]
    d = BoundarySampler(part_labels=labels, seed=11).boundary_sample_all(lm, smpl, obj, sigmas, ratios, 100000, grid_ratio=0.01)
    assert sorted(d) == sorted(["points", "dist_h", "dist_o", "parts", "pca_axis", "smpl_center", "body_kpts", "obj_center"])
    keys = ["sigma%s" % s for s in sigmas]
    for s, key, n in zip(sigmas, keys, (10100, 49490, 50500)):
        for name, dt, shape in (("points", np.float32, (n, 3)), ("dist_h", np.float32, (n,)), ("dist_o", np.float32, (n,)),
                                ("parts", np.uint8, (n,))):
            assert list(d[name]) == keys
            assert d[name][key].dtype == dt and d[name][key].shape == shape, (name, key)
        P = d["points"][key].astype(np.float64)
        bmin, bmax = BoundarySampler.get_bounds()
        grid = P[n - n // 101:]
        assert ((grid >= bmin) & (grid <= bmax)).all()
        for name, (V, F), E32 in (("dist_h", (Vh, Fh), E32h), ("dist_o", (Vo, Fo), E32o)):
            err = np.abs(d[name][key].astype(np.float64) - ref.mesh_distance_pruned(P, V, F)[0]).max()
            print("%s %s: max error %.3e (bound %.3e)" % (key, name, err, 8 * E32))
            assert err <= 8 * E32
        assert _parts_ok(P, Vh, labels, d["parts"][key]).all()
        assert np.median(d["dist_h"][key][:n - n // 101].astype(np.float64).clip(max=d["dist_o"][key][:n - n // 101])) < 2 * s
    assert d["pca_axis"].dtype == np.float32 and d["pca_axis"].shape == (3, 3)
    assert np.allclose(d["pca_axis"] @ d["pca_axis"].T, np.eye(3), atol=1e-5)
    assert d["body_kpts"].dtype == np.float32 and d["body_kpts"].shape == (25, 3)
    assert d["obj_center"].dtype == np.float32 and np.allclose(d["obj_center"], Vo.mean(0), atol=1e-6)
    assert np.array_equal(np.asarray(d["smpl_center"]), np.asarray(lm.get_smpl_center(smpl)))
    assert np.allclose(d["body_kpts"], np.asarray(lm.get_body_kpts(smpl)), atol=1e-6)
    # flip=True: the same points (same seed), the flipped labels
    s2 = BoundarySampler(part_labels=labels, seed=11)
    d2 = s2.boundary_sample_all(lm, smpl, obj, sigmas, ratios, 100000, grid_ratio=0.01, flip=True)
    for key in keys:
        assert np.array_equal(d2["points"][key], d["points"][key]) and np.array_equal(d2["dist_h"][key], d["dist_h"][key])
        assert np.array_equal(d2["parts"][key], s2.flip_part_labels(d["parts"][key]))
        assert d2["parts"][key].dtype == np.uint8
    assert any((d2["parts"][k] != d["parts"][k]).any() for k in keys)
    # given points are labelled, not drawn; the tuple of boundary_sampling
    P = d["points"][keys[1]][:3000]
    out = BoundarySampler(part_labels=labels).boundary_sampling(smpl, obj, 0.02, 3000, points=P)
    assert [o.dtype for o in out] == [np.float64, np.float32, np.float32, np.int32, np.float32, np.float32]
    assert [o.shape for o in out] == [(3000, 3), (3000,), (3000,), (3000,), (3000, 3), (3000, 3)]
    assert np.array_equal(out[0], P.astype(np.float64)) and np.array_equal(out[1], d["dist_h"][keys[1]][:3000])
    assert np.array_equal(out[2], d["dist_o"][keys[1]][:3000]) and np.array_equal(out[3], d["parts"][keys[1]][:3000])
    for nb, dist in ((out[4], out[1]), (out[5], out[2])):
        assert np.abs(np.linalg.norm(P.astype(np.float64) - nb, axis=1) - dist).max() <= 8 * max(E32h, E32o) + CLOSEST_EXTRA
    drawn = BoundarySampler(part_labels=labels, seed=2).boundary_sampling(smpl, obj, 0.02, 1000, grid_ratio=0.01)
    assert drawn[0].shape == (1010, 3) and drawn[3].shape == (1010,)


def test_train_batch_feeds_the_model(opt, scene):
    """13: targets drawn from meshes on the device go through CHORE.forward and its backward"""
    import copy
    from chore_amd.model import CHORE
    from chore_amd.preprocess.boundary_sampler import BoundarySampler
    from chore_amd.recon.assets import FileAssets
    from chore_amd.utils import synth
    from make_train_batch import train_batch
    B, N = 2, 512
    (Vh, Fh), (Vo, Fo) = body_mesh(), obj_mesh()
    sv = torch.from_numpy(np.stack([Vh, Vh + np.array([0.05, -0.02, 0.0])])).float().cuda()
    ov = torch.from_numpy(np.stack([Vo, Vo * 0.9 + 0.1])).float().cuda()
    center = torch.tensor([[0.1, 0.2, 2.2], [0.15, 0.18, 2.2]]).cuda()
    s = BoundarySampler(part_labels=FileAssets(ASSETS).part_labels(), seed=4)
    t = s.train_batch(sv, torch.from_numpy(Fh).cuda(), ov, torch.from_numpy(Fo).cuda(), center, total_samplenum=N)
    want = dict(points=((B, N, 3), torch.float32), df_h=((B, N), torch.float32), df_o=((B, N), torch.float32),
                parts_gt=((B, N), torch.int64), pca_gt=((B, 3, 3, N), torch.float32), body_center=((B, 3), torch.float32),
                obj_center=((B, 3, N), torch.float32))
    assert sorted(t) == sorted(want)
    for k, (shape, dt) in want.items():
        assert tuple(t[k].shape) == shape and t[k].dtype == dt and t[k].is_cuda and t[k].is_contiguous(), k
        assert torch.isfinite(t[k].float()).all()
    assert torch.equal(t["obj_center"], t["obj_center"][:, :, :1].expand(B, 3, N))
    assert torch.allclose(t["obj_center"][:, :, 0], ov.mean(1) - center, atol=1e-6)
    assert torch.equal(t["pca_gt"], t["pca_gt"][..., :1].expand(B, 3, 3, N))
    assert 0 <= int(t["parts_gt"].min()) and int(t["parts_gt"].max()) <= 13
    assert float(torch.minimum(t["df_h"], t["df_o"]).median()) < 0.05
    E32 = scene["E32"]["body"]
    for b in range(B):
        P = t["points"][b].cpu().numpy().astype(np.float64)
        D = ref.mesh_distance_pruned(P, sv[b].cpu().numpy().astype(np.float64), Fh)[0]
        assert np.abs(t["df_h"][b].cpu().numpy() - D).max() <= 8 * E32
    o = copy.copy(opt)
    o.compute_dtype = "fp32"
    net = CHORE(o).cuda()
    synth.load_synth_weights(net, seed=0)
    net.train(True)
    for p in net.parameters():
        p.requires_grad_(True)
    tb = train_batch(B=B, N=N)
    loss, _ = net.forward(images=torch.from_numpy(tb["images"]).cuda(), crop_center=torch.from_numpy(tb["crop_center"]).cuda(), **t)
    assert torch.isfinite(loss)
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
