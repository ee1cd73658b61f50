"""GPU: instance masks and visibility (chore_instances_fwd, chore_amd.render.rasterize_instances / face_visibility /
Renderer.visibility / Renderer.render_instances, chore_amd.preprocess.render_masks, chore_amd.recon.eval.occlusion) against the
numpy restatement tests/instances_ref.py and the colour rasteriser.  Every comparison is exact: the winners of the restatement
are bit-equal to the kernels', and everything on top of winners is integer arithmetic."""
import json
import os

import numpy as np
import pytest
import torch

import instances_ref as iref
from meshes import icosphere
from oracle import silhouette as osil

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.1, 100.0
KEYS = ("visible", "full", "face_samples", "group_samples", "face_index")


def random_tri(seed=0, B=3, V=30, Fn=40):
    """random_tri of tests/test_gpu_render.py: projected triangles in and around the view, small triangles in image 1,
    degenerate vertices in image 2, both windings (face f + Fn is face f the other way round)"""
    rs = np.random.RandomState(seed)
    v = np.concatenate([rs.uniform(-1.2, 1.2, (B, V, 2)), rs.uniform(0.5, 4.0, (B, V, 1))], -1).astype(np.float32)
    f = np.stack([np.stack([rs.choice(V, 3, replace=False) for _ in range(Fn)]) for _ in range(B)]).astype(np.int64)
    v[1, :, :2] *= 0.3
    v[2, :5] = 0.0
    return osil.vertices_to_faces(v, osil.fill_back(f))


def groups_of(tri, fn):
    """(B,F) group of every face from its index in the un-doubled list, so both windings of a face share a group"""
    B, Fn = tri.shape[:2]
    return np.broadcast_to(np.asarray([fn(f % (Fn // 2)) for f in range(Fn)], np.int32), (B, Fn)).copy()


def hip_instances(tri, group, G, size, ssaa):
    from chore_amd.render import rasterize_instances
    grp = None if group is None else torch.as_tensor(group).cuda()
    out = rasterize_instances(torch.as_tensor(np.asarray(tri, np.float32)).cuda(), grp, G, size, ssaa == 2, NEAR, FAR,
                              return_index=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def hip_alpha(tri, size, ssaa):
    from chore_amd.render import rasterize_rgbad
    t = torch.as_tensor(np.asarray(tri, np.float32)).cuda()
    tex = torch.ones(tri.shape[0], tri.shape[1], 2, 2, 2, 3, device="cuda")
    out = rasterize_rgbad(t, tex, None, size, ssaa == 2, NEAR, FAR, return_index=True)
    return out["alpha"].cpu().numpy(), out["face_index"].cpu().numpy()


def assert_equal(out, ref):
    for k in KEYS:
        assert out[k].shape == ref[k].shape and out[k].dtype == ref[k].dtype, (k, out[k].shape, out[k].dtype)
        assert np.array_equal(out[k], ref[k]), k


@pytest.fixture(scope="module")
def random_case():
    """test 1's mesh, groups and restatement, computed once"""
    tri = random_tri(0)
    grp = groups_of(tri, lambda f: f % 3)
    return tri, grp, iref.instances(tri, grp, 3, 64, 2)


def test_random_meshes(random_case):
    """1: B = 3, 80 triangles, G = 3, size 64, ssaa 2: all five outputs against the restatement, the index and the masks
    against the colour rasteriser"""
    tri, grp, ref = random_case
    counts = ref["group_samples"]
    print("visible / full samples per image and group:", counts.tolist())
    assert (0 < counts[..., 0]).all() and (counts[..., 0] < counts[..., 1]).all()          # every group partly hidden
    assert counts.tolist() == [[[6053, 11138], [2038, 11206], [7038, 13446]], [[712, 1068], [335, 972], [209, 934]],
                               [[6446, 9724], [4182, 6899], [1795, 8492]]]
    out = hip_instances(tri, grp, 3, 64, 2)
    assert_equal(out, ref)
    alpha, fim = hip_alpha(tri, 64, 2)
    assert np.array_equal(out["face_index"], fim)
    assert np.array_equal(out["visible"].sum(1), alpha)
    for g in range(3):
        sel = np.nonzero(grp[0] == g)[0]
        assert np.array_equal(out["full"][:, g], hip_alpha(tri[:, sel], 64, 2)[0]), g


@pytest.mark.parametrize("size,ssaa", [(61, 1), (61, 2), (200, 2)])
def test_tails_and_bins(size, ssaa):
    """2: a size that is no multiple of the tile at both sample counts, and 400 samples = more than one 256-sample bin; B = 1;
    one group without a group tensor, and eight groups"""
    tri = random_tri(0)[:1]
    one = hip_instances(tri, None, 1, size, ssaa)
    alpha, fim = hip_alpha(tri, size, ssaa)
    assert 0.05 < (alpha > 0).mean() < 0.95
    assert np.array_equal(one["visible"][:, 0], alpha) and np.array_equal(one["full"][:, 0], alpha)
    assert np.array_equal(one["face_index"], fim)
    assert one["group_samples"].tolist() == [[[int((fim >= 0).sum())] * 2]]
    grp = groups_of(tri, lambda f: f % 8)
    ref = iref.instances(tri, grp, 8, size, ssaa)
    assert (ref["group_samples"][..., 1] > 0).all()
    assert_equal(hip_instances(tri, grp, 8, size, ssaa), ref)


def test_occluders(random_case):
    """3: groups {0, 1, -1, 8} at G = 2: faces of the groups -1 and 8 win samples and hide what is behind them, and appear in
    no mask and no group count"""
    tri = random_case[0]
    grp = groups_of(tri, lambda f: (0, 1, -1, 8)[f % 4])
    ref = iref.instances(tri, grp, 2, 64, 2)
    member = (grp == 0) | (grp == 1)
    # the restatement itself: occluders win samples, and without them more of the groups is seen, while `full` is the same
    assert all((ref["face_samples"][b][~member[b]] > 0).any() for b in range(3))
    alone = iref.instances(np.stack([tri[b][member[b]] for b in range(3)]), np.stack([grp[b][member[b]] for b in range(3)]),
                           2, 64, 2)
    assert np.array_equal(alone["full"], ref["full"]) and (alone["visible"] >= ref["visible"]).all()
    assert (alone["group_samples"][..., 0] > ref["group_samples"][..., 0]).all()
    out = hip_instances(tri, grp, 2, 64, 2)
    assert_equal(out, ref)
    won = out["face_index"] >= 0
    assert out["group_samples"][..., 0].sum() < won.sum() == out["face_samples"].sum()


def test_empty_view():
    """4: nothing in view: masks and counts 0, the index -1"""
    tri = random_tri(0)
    tri[..., 0] += 5.0
    for ssaa in (1, 2):
        out = hip_instances(tri, groups_of(tri, lambda f: f % 3), 3, 61, ssaa)
        assert out["visible"].shape == (3, 3, 61, 61) and not out["visible"].any() and not out["full"].any()
        assert not out["face_samples"].any() and not out["group_samples"].any()
        assert out["face_index"].shape == (3, 61 * ssaa, 61 * ssaa) and (out["face_index"] == -1).all()


def test_refusals():
    """5: CHORE_EINVAL before anything is launched for G = 0, G = 9, ssaa 3 and all outputs NULL; ValueError from Python"""
    from chore_amd import _lib
    from chore_amd.render import rasterize_instances
    tri = torch.as_tensor(random_tri(0)).cuda()
    B, Fn = tri.shape[:2]
    h = _lib.handle(0)
    ws = torch.empty(_lib.lib.chore_instances_workspace_bytes(B, Fn, 1, 64, 2), dtype=torch.uint8, device="cuda")
    vis = torch.full((B, 8, 64, 64), -7.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(G, ssaa, out, tri_ptr=tri.data_ptr(), ws_ptr=ws.data_ptr()):
        return _lib.lib.chore_instances_fwd(h, tri_ptr, None, B, Fn, G, 64, ssaa, NEAR, FAR, out, None, None, None, None,
                                            ws_ptr, stream)
    einval = -1
    assert call(0, 2, vis.data_ptr()) == einval and call(9, 2, vis.data_ptr()) == einval
    assert call(1, 3, vis.data_ptr()) == einval and call(1, 2, None) == einval
    assert call(1, 2, vis.data_ptr(), tri_ptr=None) == einval and call(1, 2, vis.data_ptr(), ws_ptr=None) == einval
    assert b"chore_instances_fwd" in _lib.lib.chore_last_error(h)
    torch.cuda.synchronize()
    assert (vis == -7.0).all()                                 # nothing was launched
    assert call(1, 2, vis.data_ptr()) == 0
    for G in (0, 9):
        with pytest.raises(ValueError):
            rasterize_instances(tri, None, G, 64)
    with pytest.raises(ValueError):
        rasterize_instances(tri, torch.zeros(B, Fn - 1, dtype=torch.int32, device="cuda"), 2, 64)
    with pytest.raises(ValueError):
        rasterize_instances(tri, None, 1, 4096)                # 8192 samples


def test_repeatability_and_graph_replay(random_case):
    """6: three calls on one stream are bit-equal; one call captured into a graph and replayed twice equals the eager call"""
    from chore_amd.render import rasterize_instances
    tri, grp, ref = random_case
    t, g = torch.as_tensor(tri).cuda(), torch.as_tensor(grp).cuda()
    call = lambda: rasterize_instances(t, g, 3, 64, True, NEAR, FAR, return_index=True)      # noqa: E731
    host = lambda out: {k: v.cpu().numpy() for k, v in out.items()}                          # noqa: E731
    a = host(call())
    assert_equal(a, ref)
    for _ in range(2):
        b = host(call())
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), k
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = call()
    for _ in range(2):
        for v in out.values():
            v.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        c = host(out)
        for k in KEYS:
            assert np.array_equal(a[k], c[k]), ("replay", k)


# ---- the meshes of the demo scene (tests/test_gpu_render.py demo_scene: the body-sized ellipsoid at 2.2 m and an icosphere), with
# ---- fewer faces so that the numpy restatement takes a fraction of a second
def body_mesh():
    from chore_amd.utils.synth import uv_ellipsoid
    return uv_ellipsoid(rings=12, segments=16, center=(0.0, 0.0, 2.2))                       # 384 faces


def small_scene(sphere_centre=(0.6, 0.0, 2.2)):
    bv, bf = body_mesh()
    sv, sf = icosphere(2, 0.3, sphere_centre)
    return np.concatenate([bv, sv]).astype(np.float32), np.concatenate([bf, sf + len(bv)]).astype(np.int64)


@pytest.mark.parametrize("camera_mode", ["projection", "look_at"])
def test_renderer_visibility(camera_mode):
    """7: Renderer.visibility and mode='visibility' in both camera modes: bincount(winners at image_size) > 0, (B,2F) with
    fill_back, whatever anti_aliasing says"""
    from chore_amd import render as nr
    from chore_amd.utils.render_utils import setup_renderer
    v, f = small_scene()
    S = 64
    if camera_mode == "projection":
        make = lambda: setup_renderer(image_size=S)                                           # noqa: E731
    else:
        v = v - v.mean(0)                                     # the look_at camera looks at the origin
        make = lambda: nr.Renderer(camera_mode="look_at", image_size=S)                       # noqa: E731
    vt, ft = torch.from_numpy(v)[None].cuda(), torch.from_numpy(f)[None].cuda()
    res = {}
    for aa in (True, False):
        r = make()
        r.anti_aliasing = aa
        res[aa] = r.visibility(vt, ft)
        assert torch.equal(res[aa], r(vt, ft, mode="visibility"))
    assert res[True].dtype == torch.int32 and tuple(res[True].shape) == (1, 2 * len(f))
    assert torch.equal(res[True], res[False])
    tri = nr.vertices_to_faces(make().transform(vt), torch.cat((ft, ft.flip(-1)), 1)).cpu().numpy()
    fim = iref.winners_boxed(tri, S)
    want = np.bincount(fim[fim >= 0], minlength=2 * len(f)) > 0
    either = want.reshape(2, len(f)).any(0)                   # which winding faces the camera depends on its handedness
    assert either[:384].any() and either[384:].any() and not either.all()         # faces of both meshes are seen, not all
    assert np.array_equal(res[True][0].cpu().numpy(), want.astype(np.int32))
    assert np.array_equal(nr.face_visibility(torch.from_numpy(tri).cuda(), S)[0].cpu().numpy(), want.astype(np.int32))
    one_sided = make()
    one_sided.fill_back = False
    assert tuple(one_sided.visibility(vt, ft).shape) == (1, len(f))


# ---- masks of a frame and the occlusion of a fit --------------------------------------------------------------------
IN_FRONT, BEHIND = (0.1, 0.0, 1.5), (0.35, 0.0, 3.0)       # the object's centre: before and behind the body at 2.2 m


class M:
    def __init__(self, v, f):
        self.v, self.f = np.asarray(v, np.float64), np.asarray(f)


def frame_ref(meshes, image_size, ssaa):
    """the restatement for meshes seen through setup_renderer's camera: the projection runs on the device with the
    expressions the functions under test use, the rest in numpy"""
    from chore_amd.utils.render_utils import mesh_face_group, mesh_geometry, setup_renderer
    r = setup_renderer(image_size=image_size)
    verts, faces = mesh_geometry(meshes, "cuda:0")
    tri, grp = r._project_faces(verts, faces, (None,) * 5, mesh_face_group(meshes, "cuda:0"))
    return iref.instances(tri.cpu().numpy(), grp.cpu().numpy(), len(meshes), image_size, ssaa, winners=iref.winners_boxed)


@pytest.fixture(scope="module")
def frame_cases():
    """body + sphere before / behind it at image_size 256: meshes and the restatement at ssaa 2 and 1, computed once"""
    cases = {}
    for name, centre in (("front", IN_FRONT), ("behind", BEHIND)):
        meshes = [M(*body_mesh()), M(*icosphere(2, 0.3, centre))]
        cases[name] = (meshes, frame_ref(meshes, 256, 2), frame_ref(meshes, 256, 1))
    return cases


def test_render_masks_centroid():
    """8a: a small sphere alone: the centroid of its mask lies within one pixel of the camera's projection of its centre"""
    from chore_amd.model.camera import KinectColorCamera
    from chore_amd.preprocess import render_masks
    centre = (0.2, -0.1, 2.2)
    far_away = M(*icosphere(1, 0.05, (0.0, 0.0, -5.0)))       # behind the camera: the person's slot, never seen
    out = render_masks(far_away, M(*icosphere(3, 0.05, centre)), image_size=256)
    assert sorted(out) == ["obj_rend_full", "obj_rend_mask", "person_full", "person_mask"]
    for k, a in out.items():
        assert a.shape == (192, 256) and a.dtype == np.uint8 and set(np.unique(a)) <= {0, 255}, k
    assert not out["person_mask"].any() and not out["person_full"].any()
    assert np.array_equal(out["obj_rend_mask"], out["obj_rend_full"])
    ys, xs = np.nonzero(out["obj_rend_mask"])
    assert len(ys) >= 12                                       # radius 0.05 m at 2.2 m is 2.8 pixels
    # project_points' pixel step: pixels of the 2048-wide frame, scaled to 256; pixel i covers [i, i + 1)
    px, py = KinectColorCamera().project_screen(torch.tensor([centre]))
    want = np.array([float(px), float(py)]) * 256 / 2048 - 0.5
    got = np.array([xs.mean(), ys.mean()])
    print("centroid", got, "projection", want)
    assert np.abs(got - want).max() < 1.0


def test_render_masks_occlusion(frame_cases):
    """8b: object before the body: the object's masks agree and the person loses pixels; behind the body the reverse; the
    arrays are the restatement's and go through TrainImagePrep.prepare"""
    from chore_amd.data.train_image_prep import TrainImagePrep
    from chore_amd.preprocess import render_masks
    batch = {}
    for name, (meshes, ref, _) in frame_cases.items():
        hidden = 0 if name == "front" else 1
        vis, full = ref["group_samples"][0, hidden]
        print(name, "hidden mesh: visible / full samples", vis, full)
        assert 0.05 < vis / full < 0.95
        out = render_masks(meshes[0], meshes[1], image_size=256)
        want = {"person_mask": ref["visible"][0, 0], "person_full": ref["full"][0, 0],
                "obj_rend_mask": ref["visible"][0, 1], "obj_rend_full": ref["full"][0, 1]}
        for k, cov in want.items():
            assert np.array_equal(out[k], ((cov[:192] >= 0.5) * 255).astype(np.uint8)), (name, k)
        seen, alone = ("obj_rend_mask", "obj_rend_full") if name == "front" else ("person_mask", "person_full")
        cut, whole = ("person_mask", "person_full") if name == "front" else ("obj_rend_mask", "obj_rend_full")
        assert np.array_equal(out[seen], out[alone]) and out[seen].any()
        assert (out[cut] <= out[whole]).all() and (out[cut] < out[whole]).any()
        batch[name] = out
    prep = TrainImagePrep(crop_size=150, phase="test")
    rgb = np.full((2, 192, 256, 3), 128, np.uint8)
    res = prep.prepare(rgb, [batch[n]["person_mask"] for n in batch], [batch[n]["obj_rend_mask"] for n in batch])
    assert tuple(res["images"].shape) == (2, 5, 512, 512) and torch.isfinite(res["images"]).all()


def test_occlusion_counts(frame_cases):
    """9a: the counts of `occlusion` are the restatement's at one sample per pixel over the frame rows; the object fraction is
    exactly 1 when the object is before the body; occlusion_report transforms the template like penetration_report"""
    from chore_amd.recon.eval.occlusion import MIN_VISIBLE, occlusion
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    assert MIN_VISIBLE == 0.30
    names = ("front", "behind")
    body = frame_cases["front"][0][0]
    obj_f = frame_cases["front"][0][1].f
    sv = torch.as_tensor(np.stack([body.v, body.v]), dtype=torch.float32).cuda()
    ov = torch.as_tensor(np.stack([frame_cases[n][0][1].v for n in names]), dtype=torch.float32).cuda()
    out = occlusion(sv, torch.as_tensor(body.f).cuda(), ov, torch.as_tensor(obj_f).cuda(), image_size=256)
    for i, n in enumerate(names):
        ref = frame_cases[n][2]
        for g, who in enumerate(("body", "object")):
            for key, per_sample in (("visible", ref["vis"]), ("full", ref["cov"])):
                # ssaa 1: sample row y is image row 255 - y, the frame is the upper 192 image rows
                want = int(per_sample[0, g][256 - 192:].sum())
                t = out["%s_%s" % (who, key)]
                assert t.dtype == torch.int64 and tuple(t.shape) == (2,) and int(t[i]) == want > 0, (n, who, key)
            frac = out[who + "_fraction"]
            assert frac.dtype == torch.float64
            assert float(frac[i]) == int(out[who + "_visible"][i]) / int(out[who + "_full"][i])
    assert float(out["object_fraction"][0]) == 1.0 and float(out["body_fraction"][0]) < 1.0
    assert float(out["object_fraction"][1]) < 1.0 and float(out["body_fraction"][1]) == 1.0
    # nothing of the object in view: the fraction is NaN
    gone = occlusion(sv[:1], body.f, ov[:1] + torch.tensor([50.0, 0.0, 0.0]).cuda(), obj_f, image_size=256)
    assert int(gone["object_full"][0]) == 0 and torch.isnan(gone["object_fraction"][0]) and float(gone["body_fraction"][0]) == 1.0
    # the fitter's report: the template at the origin, moved to the two places
    ov0, _ = icosphere(2, 0.3)
    fitter = ReconFitterBase.from_parts(scan_verts=np.asarray(ov0, np.float32), scan_faces=obj_f)
    R, t, s = torch.eye(3).cuda()[None].repeat(2, 1, 1), torch.tensor([IN_FRONT, BEHIND]).cuda(), torch.ones(2).cuda()
    rep = fitter.occlusion_report(sv, torch.as_tensor(body.f).cuda(), R, t, s)
    assert sorted(rep) == sorted(out)
    for k in ("body_full", "object_visible"):
        assert (rep[k] > 0).all()
    assert float(rep["object_fraction"][0]) == 1.0 and float(rep["body_fraction"][1]) == 1.0


def test_report_occlusion_flag(tmp_path):
    """9b: save_outputs of a fitter on SyntheticAssets writes k1.occlusion.json only with the switch on; the PLY and PKL files
    are byte-equal either way"""
    from chore_amd.recon.assets import SyntheticAssets
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    paths = [os.path.join("data", "seq%d" % k, "t0001.000", "k1.color.jpg") for k in range(2)]
    files = {}
    for flag in (False, True):
        out_dir = str(tmp_path / ("on" if flag else "off"))
        fitter = ReconFitterBase(None, device="cuda:0", obj_name="synthetic", outpath=out_dir, assets=SyntheticAssets(0))
        assert fitter.REPORT_OCCLUSION is False
        if flag:
            fitter.REPORT_OCCLUSION = True
        smpl = fitter.get_smpl_init(paths, torch.tensor([[0.0, 0.0, 2.2], [0.1, 0.0, 2.2]]))
        obj_R = (torch.eye(3)[None].repeat(2, 1, 1) + 0.01 * torch.arange(18.0).reshape(2, 3, 3)).cuda()
        obj_t = torch.tensor([[0.0, 0.0, 1.6], [40.0, 0.0, 2.2]]).cuda()          # frame 0: before the body; frame 1: out of view
        obj_s = torch.ones(2).cuda()
        torch.manual_seed(3)                                                      # save_outputs perturbs the rotation parameter
        fitter.save_outputs(smpl, obj_R, obj_t, paths, "test", 1, obj_s)
        files[flag] = {}
        for root, _, names in os.walk(out_dir):
            for n in names:
                files[flag][os.path.relpath(os.path.join(root, n), out_dir)] = open(os.path.join(root, n), "rb").read()
    assert len(files[False]) == 8 and all(n.endswith((".ply", ".pkl")) for n in files[False])
    extra = sorted(set(files[True]) - set(files[False]))
    assert extra == [os.path.join("seq%d" % k, "t0001.000", "test", "k1.occlusion.json") for k in range(2)]
    for n, data in files[False].items():
        assert files[True][n] == data, n
    reps = [json.loads(files[True][n]) for n in extra]
    print("occlusion of the two frames:", reps)
    for r in reps:
        assert sorted(r) == ["body_fraction", "body_full", "body_visible", "object_evaluated", "object_fraction", "object_full",
                             "object_visible"]
    assert reps[0]["object_fraction"] == 1.0 and reps[0]["object_evaluated"] is True and 0 < reps[0]["body_fraction"] < 1
    assert reps[0]["object_visible"] == reps[0]["object_full"] > 0 and 0 < reps[0]["body_visible"] < reps[0]["body_full"]
    assert reps[1]["object_full"] == 0 and reps[1]["object_fraction"] is None and reps[1]["object_evaluated"] is False
    assert reps[1]["body_fraction"] == 1.0
