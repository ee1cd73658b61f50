"""GPU: the signed mesh distance (chore_mesh_sdf_fwd; `winding`, `inside`, `signed` of chore_amd.preprocess.mesh_distance) and
the penetration report built on it, against the float64 restatement of the generalized winding number in
tests/mesh_sign_ref.py and known answers.

The bound of every winding-number comparison is 8 x W32, W32 = the largest |float32 - float64| of the restatement itself on
the case's own points (computed here once per run, the `cases` fixture; the convention of tests/test_gpu_mesh_dist.py with its
8 x E32).  Shapes: one point tile of the kernel is 512 points, one LDS tile 128 faces, the number of face chunks follows
md_chunks (csrc/mesh_dist.hip) -- 12 faces: one partial tile, one chunk; 1 728: 14 chunks, the last tile half filled; 320:
3 chunks; 152: an open mesh; 13 776 at N = 513: the chunk cap of 64 and a second point tile that holds one point."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_dist_ref as ref
import mesh_sign_ref as sref
from meshes import icosphere

pytestmark = pytest.mark.gpu

BOX = ((-0.3, -0.2, 2.0), (0.4, 0.5, 2.6))
CLOSED = ("box1", "box12", "ico2", "body")
NAMES = ("box1", "box12", "ico2", "hemi", "body")
UNSIGNED = ("dist", "face_idx", "closest", "vert_idx")


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def gpu(P, V, F, want, **kw):
    from chore_amd.preprocess import mesh_distance
    out = mesh_distance(dev(P, np.float32), dev(V, np.float32), dev(F, np.int32), want, **kw)
    return {k: v.cpu().numpy() for k, v in zip(want, out)}


def _case(V, F, P):
    V, P = f32(V), f32(P)
    w64, w32 = sref.winding(P, V, F), sref.winding(P, V, F, np.float32)
    return dict(V=V, F=F, P=P, w64=w64, W32=float(np.abs(w32.astype(np.float64) - w64).max()), D64=ref.mesh_distance_pruned(P, V, F)[0],
                delta=1e-5 * float(np.linalg.norm(V.max(0) - V.min(0))))


@pytest.fixture(scope="module")
def cases():
    """meshes, points and the float64 / float32 restatement of every case, computed once and left unchanged"""
    from chore_amd.utils.synth import uv_ellipsoid
    Pbox = np.random.RandomState(1).rand(2400, 3) * 1.6 + np.array([-0.8, -0.7, 1.5])          # the set of test_known_box
    ico = icosphere(2, 0.35, (0.45, 0.1, 2.3))
    Pico = ref.sampler_points([(f32(ico[0]), ico[1])], 170, 30, np.random.RandomState(0))[0]
    body = uv_ellipsoid(center=(0.1, 0.2, 2.2))
    Pbody = ref.sampler_points([(f32(body[0]), body[1])], 100, 71, np.random.RandomState(2))[0]
    c = {"box1": _case(*sref.oriented_box(BOX[0], BOX[1], 1), Pbox), "box12": _case(*sref.oriented_box(BOX[0], BOX[1], 12), Pbox),
         "ico2": _case(*ico, Pico), "hemi": _case(*sref.hemisphere(2, 0.35, (0.45, 0.1, 2.3)), Pico), "body": _case(*body, Pbody)}
    assert [len(c[k]["F"]) for k in NAMES] == [12, 1728, 320, 152, 13776]
    assert [len(c[k]["P"]) for k in NAMES] == [2400, 2400, 600, 600, 513]
    for k in NAMES:
        print("%s: W32 %.3e" % (k, c[k]["W32"]))
        assert 0 < c[k]["W32"] < 1e-4
    return c


def check_winding(c, w, what, sign=1.0):
    """condition 1: every point within 8 W32 of the float64 value"""
    err = np.abs(w.astype(np.float64) - sign * c["w64"]).max()
    print("%s: W32 %.3e  bound %.3e  kernel max |winding - w64| %.3e (%.2f W32)" % (what, c["W32"], 8 * c["W32"], err, err / c["W32"]))
    assert np.isfinite(w).all() and err <= 8 * c["W32"], (what, err, 8 * c["W32"])


def check_inside_closed(c, inside, what):
    """condition 2: equal to |w64| > 0.5 at every point at least delta from the surface; at most 1 % are nearer"""
    keep = c["D64"] >= c["delta"]
    print("%s: %d of %d points nearer than delta = %.3e left out" % (what, (~keep).sum(), len(keep), c["delta"]))
    assert (~keep).sum() <= 0.01 * len(keep)
    assert np.array_equal(inside[keep], (np.abs(c["w64"]) > 0.5)[keep]), what
    return keep


@pytest.mark.parametrize("name", NAMES)
def test_winding_and_inside(cases, name):
    """1, 2, 3: winding within the bound everywhere; inside on the closed meshes (on the boxes also against lo < p < hi) and,
    on the hemisphere, wherever the float64 value is farther than the bound from the threshold"""
    c = cases[name]
    out = gpu(c["P"], c["V"], c["F"], ("winding", "inside"))
    assert out["winding"].dtype == np.float32 and out["inside"].dtype == np.bool_
    assert out["winding"].shape == out["inside"].shape == (len(c["P"]),)
    check_winding(c, out["winding"], name)
    if name in CLOSED:
        keep = check_inside_closed(c, out["inside"], name)
        assert 0 < out["inside"].sum() < len(keep)
        assert np.abs(c["w64"] - np.rint(c["w64"])).max() <= 1e-12           # integers: the mesh is closed
        if name.startswith("box"):
            lo, hi = f32(BOX[0]), f32(BOX[1])
            assert np.array_equal(out["inside"][keep], ((c["P"] > lo) & (c["P"] < hi)).all(1)[keep])
    else:
        sure = np.abs(np.abs(c["w64"]) - 0.5) > 8 * c["W32"]
        print("%s: %d of %d points farther than the bound from the threshold" % (name, sure.sum(), len(sure)))
        assert sure.sum() >= 0.99 * len(sure)
        assert np.array_equal(out["inside"][sure], (np.abs(c["w64"]) > 0.5)[sure])
        frac = np.abs(c["w64"] - np.rint(c["w64"]))
        assert (frac > 0.01).sum() > 0.5 * len(frac)                          # an open mesh: fractional values


@pytest.mark.parametrize("name", NAMES)
def test_signed_and_the_unsigned_outputs(cases, name):
    """4, 5: signed is -dist inside and +dist elsewhere, bit for bit; sign_mode='winding' is (1 - 2 winding) dist in float32;
    dist, face_idx, closest, vert_idx of a call that also asks for winding have the bits of a call that does not"""
    c = cases[name]
    plain = gpu(c["P"], c["V"], c["F"], UNSIGNED)
    out = gpu(c["P"], c["V"], c["F"], UNSIGNED + ("winding", "inside", "signed"))
    for k in UNSIGNED:
        assert np.array_equal(out[k], plain[k]), (name, k)
    assert out["signed"].dtype == np.float32
    assert np.array_equal(out["signed"].view(np.uint32), np.where(out["inside"], -out["dist"], out["dist"]).view(np.uint32))
    assert np.array_equal(np.abs(out["signed"]), out["dist"])
    frac = gpu(c["P"], c["V"], c["F"], ("signed", "winding", "dist"), sign_mode="winding")
    assert np.array_equal(frac["winding"], out["winding"]) and np.array_equal(frac["dist"], out["dist"])
    want = (np.float32(1) - np.float32(2) * frac["winding"]) * frac["dist"]
    assert want.dtype == np.float32 and np.array_equal(frac["signed"].view(np.uint32), want.view(np.uint32))
    only = gpu(c["P"], c["V"], c["F"], ("signed",))
    assert np.array_equal(only["signed"].view(np.uint32), out["signed"].view(np.uint32))


def test_names_and_modes_are_checked():
    from chore_amd.preprocess import mesh_distance
    p, v, f = torch.zeros(4, 3).cuda(), torch.eye(3).cuda(), torch.tensor([[0, 1, 2]]).cuda()
    with pytest.raises(ValueError):
        mesh_distance(p, v, f, ("signed",), sign_mode="igl")
    with pytest.raises(ValueError):
        mesh_distance(p, v, f, ("sign",))
    w = mesh_distance(p, v, f, "winding")
    assert w.shape == (4,) and w.dtype == torch.float32


@pytest.mark.parametrize("N", [1, 511])
def test_shapes_points(cases, N):
    """N = 1 and N = 511 on ico2: the first N points of the case"""
    c = cases["ico2"]
    out = gpu(c["P"][:N], c["V"], c["F"], ("winding", "inside", "dist"))
    sub = dict(c, w64=c["w64"][:N], D64=c["D64"][:N])
    assert out["winding"].shape == (N,)
    check_winding(sub, out["winding"], "ico2 N=%d" % N)
    keep = sub["D64"] >= c["delta"]
    assert np.array_equal(out["inside"][keep], (np.abs(sub["w64"]) > 0.5)[keep])


def test_shapes_batched(cases):
    """B = 2 on ico2, the second item's vertices shifted by (0.3, 0, 0): every item against its own mesh"""
    from chore_amd.preprocess import mesh_distance
    c = cases["ico2"]
    V2 = f32(c["V"] + np.array([0.3, 0.0, 0.0]))
    w2 = sref.winding(c["P"], V2, c["F"])
    W32b = float(np.abs(sref.winding(c["P"], V2, c["F"], np.float32).astype(np.float64) - w2).max())
    names = ("winding", "inside", "signed", "dist")
    out = mesh_distance(dev(np.stack([c["P"], c["P"]]), np.float32), dev(np.stack([c["V"], V2]), np.float32), dev(c["F"], np.int32),
                        names)
    assert [tuple(o.shape) for o in out] == [(2, 600)] * 4
    assert [o.dtype for o in out] == [torch.float32, torch.bool, torch.float32, torch.float32]
    w = out[0].cpu().numpy()
    check_winding(c, w[0], "B=2 item 0")
    check_winding(dict(w64=w2, W32=W32b), w[1], "B=2 item 1")
    assert not np.array_equal(w[0], w[1])
    ins = out[1].cpu().numpy()
    sg, d = out[2].cpu().numpy(), out[3].cpu().numpy()
    assert np.array_equal(sg.view(np.uint32), np.where(ins, -d, d).view(np.uint32))


def test_reproducible_and_capturable(cases):
    """6: two eager calls and a hipGraph replay of the signed call give the same bits"""
    from chore_amd.preprocess import mesh_distance
    c = cases["body"]
    p, v, f = dev(c["P"], np.float32), dev(c["V"], np.float32), dev(c["F"], np.int32)
    names = UNSIGNED + ("winding", "inside", "signed")

    def call():
        return mesh_distance(p, v, f, names)
    a, b = call(), call()
    for k, x, y in zip(names, a, b):
        assert torch.equal(x, y), k
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        cc = call()
    for _ in range(2):
        for t in cc:
            t.fill_(1) if t.dtype == torch.bool else t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k, x, y in zip(names, a, cc):
            assert torch.equal(x, y), k


def test_degenerate_faces(cases):
    """7: 200 degenerate faces, (0,0,0) and (i,i,j) mixed, appended to ico2 change nothing; points exactly on vertices and on
    face centres give finite output"""
    c = cases["ico2"]
    rs = np.random.RandomState(4)
    i, j = rs.randint(0, len(c["V"]), 100), rs.randint(0, len(c["V"]), 100)
    deg = np.concatenate([np.zeros((100, 3), np.int64), np.stack([i, i, j], 1)])[rs.permutation(200)]
    F = np.concatenate([c["F"], deg])
    base = gpu(c["P"], c["V"], c["F"], ("winding", "inside"))
    out = gpu(c["P"], c["V"], F, ("winding", "inside", "signed", "dist"))
    assert all(np.isfinite(v).all() for v in out.values())
    check_winding(c, out["winding"], "ico2 + 200 degenerate faces")
    assert np.array_equal(out["inside"], base["inside"])
    # degenerate faces alone: exactly 0 everywhere, also for points on their vertices
    Pv = f32(np.concatenate([c["P"][:50], c["V"]]))
    alone = gpu(Pv, c["V"], deg, ("winding", "inside"))
    assert (alone["winding"] == 0).all() and not alone["inside"].any()
    # points on vertices and on face centres of the mesh itself
    Pon = f32(np.concatenate([c["V"], c["V"][c["F"]].mean(1)]))
    on = gpu(Pon, c["V"], F, ("winding", "inside", "signed", "dist") + UNSIGNED[1:])
    assert all(np.isfinite(v).all() for v in on.values())


def test_reversed_faces(cases):
    """8: every face of ico2 reversed: the negated winding number, the same inside"""
    c = cases["ico2"]
    base = gpu(c["P"], c["V"], c["F"], ("inside",))
    out = gpu(c["P"], c["V"], c["F"][:, ::-1], ("winding", "inside", "signed"))
    check_winding(c, out["winding"], "ico2 reversed", sign=-1.0)
    assert np.array_equal(out["inside"], base["inside"]) and out["winding"].min() < -0.99
    assert (out["signed"][out["inside"]] <= 0).all()


def test_penetration():
    """9: vertices of a small sphere inside a large one against the float64 restatement; a sphere far away gives zeros"""
    from chore_amd.recon.eval.penetration import penetration
    from test_gpu_mesh_dist import e32_of
    VA, FA = icosphere(3, 1.0)
    VB0, FB = icosphere(2, 0.5, (1.2, 0.0, 0.0))
    VB1, _ = icosphere(2, 0.5, (3.0, 0.0, 0.0))
    VA, VB0, VB1 = f32(VA), f32(VB0), f32(VB1)
    inside = np.abs(sref.winding(VB0, VA, FA)) > 0.5
    D64 = ref.mesh_distance_brute(VB0, VA, FA)[0]
    E32 = e32_of(VB0, VA, FA)
    assert 10 < inside.sum() < len(VB0) - 10 and not (np.abs(sref.winding(VB1, VA, FA)) > 0.5).any()
    out = penetration(dev(np.stack([VA, VA]), np.float32), dev(FA, np.int32), dev(np.stack([VB0, VB1]), np.float32), dev(FB, np.int32))
    assert sorted(out) == ["count", "frac", "max_depth", "mean_depth"]
    assert all(v.is_cuda and tuple(v.shape) == (2,) for v in out.values())
    out = {k: v.cpu().numpy() for k, v in out.items()}
    print("penetration: count %s frac %s max %s mean %s  (E32 %.3e)"
          % (out["count"], out["frac"], out["max_depth"], out["mean_depth"], E32))
    assert out["count"][0] == inside.sum() and out["count"][1] == 0
    assert out["frac"][0] == np.float32(inside.sum()) / np.float32(len(VB0)) and out["frac"][1] == 0
    assert abs(float(out["max_depth"][0]) - D64[inside].max()) <= 8 * E32
    assert abs(float(out["mean_depth"][0]) - D64[inside].mean()) <= 8 * E32
    assert out["max_depth"][1] == 0 and out["mean_depth"][1] == 0
    one = penetration(dev(VA, np.float32), dev(FA, np.int32), dev(VB0, np.float32))                # unbatched
    assert int(one["count"][0]) == inside.sum()


def test_penetration_report_open_and_closed_template():
    """9: object-in-body always; body-in-object only when the template is a closed mesh"""
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    VA, FA = icosphere(3, 1.0)
    body_v, body_f = dev(f32(VA)[None], np.float32), dev(FA, np.int64)
    R, t, s = torch.eye(3).cuda()[None], torch.zeros(1, 3).cuda(), torch.ones(1).cuda()
    Vh, Fh = sref.hemisphere(2, 0.5, (1.2, 0.0, 0.0))
    fitter = ReconFitterBase.from_parts(scan_verts=f32(Vh), scan_faces=Fh)
    rep = fitter.penetration_report(body_v, body_f, R, t, s)
    assert sorted(rep) == ["body_in_object", "object_in_body"] and rep["body_in_object"] is None
    inside = np.abs(sref.winding(f32(Vh), f32(VA), FA)) > 0.5
    assert int(rep["object_in_body"]["count"][0]) == inside.sum() > 0
    Vc, Fc = icosphere(2, 0.5, (1.2, 0.0, 0.0))
    closed = ReconFitterBase.from_parts(scan_verts=f32(Vc), scan_faces=Fc)
    rep = closed.penetration_report(body_v, body_f, R, t, s)
    assert int(rep["object_in_body"]["count"][0]) == inside.sum()                   # the same vertices, the faces do not matter
    back = np.abs(sref.winding(f32(VA), f32(Vc), Fc)) > 0.5
    assert rep["body_in_object"] is not None and int(rep["body_in_object"]["count"][0]) == back.sum() > 0
    # the transformation is compute_collision_loss's: rotate, translate, then scale
    moved = closed.penetration_report(body_v, body_f, R, torch.tensor([[5.0, 0.0, 0.0]]).cuda(), s)
    assert int(moved["object_in_body"]["count"][0]) == 0 and float(moved["object_in_body"]["mean_depth"][0]) == 0


def test_report_penetration_flag(tmp_path):
    """10: save_outputs of a fitter on SyntheticAssets writes the JSON only with the flag set; PLY and pkl bytes are the same"""
    from chore_amd.recon.assets import SyntheticAssets
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    paths = [os.path.join("data", "seq%d" % k, "t0001.000", "k1.color.jpg") for k in range(2)]
    files = {}
    for flag in (False, True):
        out_dir = str(tmp_path / ("on" if flag else "off"))
        fitter = ReconFitterBase(None, device="cuda:0", obj_name="synthetic", outpath=out_dir, assets=SyntheticAssets(0))
        assert fitter.REPORT_PENETRATION is False
        if flag:
            fitter.REPORT_PENETRATION = True
        trans = torch.tensor([[0.0, 0.0, 2.2], [0.1, 0.0, 2.2]])
        smpl = fitter.get_smpl_init(paths, trans)
        obj_R = (torch.eye(3)[None].repeat(2, 1, 1) + 0.01 * torch.arange(18.0).reshape(2, 3, 3)).cuda()
        obj_t = torch.tensor([[0.0, 0.0, 2.2], [4.0, 0.0, 2.2]]).cuda()          # frame 0: in the body; frame 1: far from it
        obj_s = torch.ones(2).cuda()
        torch.manual_seed(3)                                                      # save_outputs perturbs the rotation parameter
        fitter.save_outputs(smpl, obj_R, obj_t, paths, "test", 1, obj_s)
        files[flag] = {}
        for root, _, names in os.walk(out_dir):
            for n in names:
                files[flag][os.path.relpath(os.path.join(root, n), out_dir)] = open(os.path.join(root, n), "rb").read()
    assert len(files[False]) == 8 and all(n.endswith((".ply", ".pkl")) for n in files[False])
    extra = sorted(set(files[True]) - set(files[False]))
    assert extra == [os.path.join("seq%d" % k, "t0001.000", "test", "k1.penetration.json") for k in range(2)]
    for n, data in files[False].items():
        assert files[True][n] == data, n
    reps = [json.loads(files[True][n]) for n in extra]
    for r in reps:
        assert sorted(r) == ["body_in_object", "object_in_body"]
        for d in r.values():
            assert sorted(d) == ["count", "frac", "max_depth", "mean_depth"]         # the synthetic template is closed: both directions
    print("penetration of the two frames:", reps)
    assert reps[0]["object_in_body"]["count"] > 0 and reps[0]["object_in_body"]["max_depth"] > 0
    assert reps[1]["object_in_body"]["count"] == 0 and reps[1]["body_in_object"]["count"] == 0
