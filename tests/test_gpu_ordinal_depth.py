"""GPU: the ordinal depth term (csrc/ordinal_depth.hip: chore_sil_depth, chore_ordinal_depth_fwd / _bwd), SilLossROI.set_occluder /
depth_loss and the fitter's ORDINAL_DEPTH_TERM / REPORT_DEPTH_ORDER, against the merged kernels (chore_render_fwd / _bwd) and the
float64 restatement tests/ordinal_depth_ref.py.  The winner map is always chore_silhouette_fwd's own, so no pixel is left out.

Shapes: B in {1, 3}; S = 64 and S = 40 (partial 16 x 16 tiles; 1 600 pixels are no multiple of a 256-pixel block; the silhouette
rasteriser takes 40 as it is); a 12-face box and the fixture's 40-vertex template, both windings; occluder: the rigid body of
tests/fit_harness.py (synthetic SMPL-H vertices, 13 776 faces), moved to a depth of 4.5 so that a difference beyond c = 2 fits
in front of it.  Frame 0: identity rotation, the object's centre at the median depth of the body's surface (it straddles it), and
the object face that wins most pixels is part of the occluder too (exactly equal depths); frame 1: rotated, 3.2 in front of
that surface (every difference exceeds c); frame 2: rotated, straddling, but the masks label nothing (no violating pixel)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import ordinal_depth_ref as odr
from conftest import golden

pytestmark = pytest.mark.gpu

FAR, NEAR = 100.0, 0.1
BODY_Z = 4.5


def dev(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _body():
    """(3,6890,3) float32 body vertices around depth BODY_Z and the (13776,3) faces of tests/fit_harness.py"""
    from chore_amd.lib_smpl.wrapper_pytorch import SMPLPyTorchWrapperBatch
    from chore_amd.utils import synth
    from fit_harness import fit_case, smplh_faces
    c = fit_case(3)
    model = synth.synth_smplh_model(0)
    faces = smplh_faces()
    model["f"] = faces
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy())      # noqa: E731
    smpl = SMPLPyTorchWrapperBatch(model, 3, betas=t_(c["betas"]), pose=t_(c["pose"]), trans=t_(c["trans"])).cuda()
    with torch.no_grad():
        v = smpl()[0].cpu().numpy().astype(np.float32)
    v[..., 2] += np.float32(BODY_Z) - v[..., 2].mean(1, keepdims=True)
    return v, faces


def _object(kind):
    if kind == "box":
        return odr.box_verts((0.45, 0.35, 0.2)), odr.BOX_FACES
    g = golden("sil_project.npz")
    v = g["verts"].astype(np.float64)
    return ((v - v.mean(0)) * 0.8).astype(np.float32), g["faces"].astype(np.int64)


def _roi_K(body):
    """(B,3,3) intrinsics (image side 1) that put the body's centre in the middle and its largest extent over 0.8 of the view"""
    Ks = []
    for v in body:
        c = 0.5 * (v.min(0) + v.max(0))
        f = 0.8 * c[2] / float((v.max(0) - v.min(0))[:2].max())
        Ks.append([[f, 0, 0.5 - f * c[0] / c[2]], [0, f, 0.5 - f * c[1] / c[2]], [0, 0, 1]])
    return np.asarray(Ks, np.float32)


def _centre(v):
    return 0.5 * (v.min(0) + v.max(0))


@functools.lru_cache(maxsize=None)
def scene(B, S, kind):
    """the term on the device, its inputs downloaded, and the float64 reference -- built once per case"""
    from chore_amd import _lib
    from chore_amd.recon.obj_pose_roi import SilLossROI
    body, bfaces = _body()
    body = body[:B]
    ov, of = _object(kind)
    image_ref, keep = odr.block_masks(B, S, 11 + S)
    if B > 2:
        image_ref[2], keep[2] = 0, 1                            # frame 2: free background everywhere
    sil = SilLossROI.from_crops(image_ref > 0.5, keep < 0.5, _roi_K(body), ov, of)
    assert np.array_equal(sil.image_ref.cpu().numpy(), image_ref) and np.array_equal(sil.keep_mask.cpu().numpy(), keep)
    # where the body's surface is: the median depth of the body alone over each frame's view
    sil.set_occluder(dev(body), bfaces)
    occ0 = sil.occ_depth.cpu().numpy()
    surface = [float(np.median(o[o < FAR])) for o in occ0]
    Rs, ts = [], []
    for b in range(B):
        c = _centre(body[b])
        Rs.append(np.eye(3, dtype=np.float32) if b == 0 else odr.rot_xyz(0.5 + b, 0.4, 0.2 * b))
        ts.append(np.array([c[0] + 0.02, c[1] - 0.03, surface[b] - (3.2 if b == 1 else 0.0)], np.float32))
    R, t, s = dev(np.stack(Rs)), dev(np.stack(ts)), torch.ones(B).cuda()
    with torch.no_grad():
        _, tri, fim = sil.render_parts(R, t, s)
    fim_h = fim.cpu().numpy()
    ids, n = np.unique(fim_h[0][fim_h[0] >= 0] % len(of), return_counts=True)
    shared = ids[np.argsort(-n)[:1]]
    # the occluder: the body, and six more vertices (two faces): in frame 0 the first three are the placed corners of the shared
    # object face (v + t in float32 is what the placement kernel computes for the identity rotation and unit scale), all others
    # copies of vertex 0 (zero-area faces)
    extra = np.repeat(body[:, :1], 6, 1)
    placed0 = (dev(ov) + t[0]).cpu().numpy()
    extra[0, :3] = placed0[of[shared[0]]]
    occ_v = np.concatenate([body, extra], 1)
    V = body.shape[1]
    occ_f = np.concatenate([bfaces, np.arange(V, V + 6).reshape(2, 3)])
    sil.set_occluder(dev(occ_v), occ_f)
    h = _lib.handle(0)
    d_obj = torch.empty(B, S, S, device="cuda")
    _lib.check(_lib.lib.chore_sil_depth(h, tri.data_ptr(), fim.data_ptr(), B, tri.shape[1], S, FAR, 1, d_obj.data_ptr(), _stream()), h,
               "chore_sil_depth")
    occ = sil.occ_depth.cpu().numpy()
    ref = odr.forward(tri.cpu().numpy(), fim_h, occ, image_ref, keep, d32=d_obj.cpu().numpy())
    return dict(sil=sil, R=R, t=t, s=s, tri=tri, fim=fim, tri_h=tri.cpu().numpy(), fim_h=fim_h, occ=occ, d_obj=d_obj, ref=ref,
                image_ref=image_ref, keep=keep, n_obj_faces=len(of), shared=shared)


CASES = [(B, S, kind) for B in (1, 3) for S in (64, 40) for kind in ("box", "template")]


def _render_depth(tri, S):
    """depth (B,S,S) and sample_face_index (B,S,S) of chore_render_fwd at ssaa 1"""
    from chore_amd import _lib
    h = _lib.handle(0)
    B, Fn = tri.shape[:2]
    tex = torch.zeros(B, Fn, 2, 2, 2, 3, device="cuda")
    rgb = torch.empty(B, 3, S, S, device="cuda")
    depth, alpha = torch.empty(B, S, S, device="cuda"), torch.empty(B, S, S, device="cuda")
    sfi = torch.empty(B, S, S, dtype=torch.int32, device="cuda")
    ws = torch.empty(_lib.lib.chore_render_workspace_bytes(B, Fn, S, 1), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.chore_render_fwd(h, tri.data_ptr(), tex.data_ptr(), None, B, Fn, 2, S, 1, NEAR, FAR, 1e-3,
                                         (ctypes.c_float * 3)(0, 0, 0), rgb.data_ptr(), depth.data_ptr(), alpha.data_ptr(),
                                         sfi.data_ptr(), ws.data_ptr(), _stream()), h, "chore_render_fwd")
    return depth, sfi


def _fwd(c):
    from chore_amd import _lib
    h = _lib.handle(0)
    sil, tri, fim = c["sil"], c["tri"], c["fim"]
    B, Fn = tri.shape[:2]
    S = fim.shape[1]
    sums = torch.full((B,), float("nan"), device="cuda")
    coef = torch.full((B, S, S), float("nan"), device="cuda")
    counts = torch.full((B, 4), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(_lib.lib.chore_ordinal_depth_workspace_bytes(B, S), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.chore_ordinal_depth_fwd(h, tri.data_ptr(), fim.data_ptr(), sil.occ_depth.data_ptr(), sil.image_ref.data_ptr(),
                                                sil.keep_mask.data_ptr(), B, Fn, S, FAR, odr.C, sums.data_ptr(), coef.data_ptr(),
                                                counts.data_ptr(), ws.data_ptr(), _stream()), h, "chore_ordinal_depth_fwd")
    return sums, coef, counts


def _bwd(c, coef, g):
    from chore_amd import _lib
    h = _lib.handle(0)
    tri, fim = c["tri"], c["fim"]
    B, Fn = tri.shape[:2]
    gt = torch.full((B, Fn, 3, 3), float("nan"), device="cuda")
    _lib.check(_lib.lib.chore_ordinal_depth_bwd(h, tri.data_ptr(), fim.data_ptr(), coef.data_ptr(), g.data_ptr(), B, Fn, fim.shape[1],
                                                gt.data_ptr(), _stream()), h, "chore_ordinal_depth_bwd")
    return gt


@pytest.mark.parametrize("B,S,kind", CASES)
def test_sil_depth_is_the_render_depth(B, S, kind):
    """1: chore_sil_depth on chore_silhouette_fwd's winner map equals the depth image of chore_render_fwd at ssaa 1 bit for bit
    (object and occluder), holds far_z exactly where nothing won, and its unflipped form is the flipped one with the rows
    reversed; the winner maps of the two rasterisers are equal as integers"""
    from chore_amd import _lib
    c = scene(B, S, kind)
    sil = c["sil"]
    for name, tri, fim, got in (("object", c["tri"], c["fim"], c["d_obj"]), ("occluder", sil._occ_tri, sil._occ_fim, sil.occ_depth)):
        want, sfi = _render_depth(tri, S)
        assert torch.equal(sfi, fim), name
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, int((got != want).sum()))
        hit = (fim >= 0).flip(1)
        assert hit.any() and (got[~hit] == FAR).all() and (got[hit] < FAR).all() and (got[hit] > NEAR).all()
    h = _lib.handle(0)
    plain = torch.empty_like(c["d_obj"])
    _lib.check(_lib.lib.chore_sil_depth(h, c["tri"].data_ptr(), c["fim"].data_ptr(), B, c["tri"].shape[1], S, FAR, 0, plain.data_ptr(),
                                        _stream()), h, "chore_sil_depth")
    assert torch.equal(plain.flip(1), c["d_obj"])
    print("B %d S %d %s: object covers %d pixels, occluder %d" % (B, S, kind, int((c["fim"] >= 0).sum()), int((sil._occ_fim >= 0).sum())))


@pytest.mark.parametrize("B,S,kind", CASES)
def test_forward_against_float64(B, S, kind):
    """2: counts equal to the restatement's as integers; coef and the sums within derived bounds; two calls bit-equal.

    Bounds.  The restatement evaluates the depth rule (tri_setup: 4 operations per pixel coordinate, 5 for the determinant, 1 or
    3 per cofactor, 1 division per inverse entry; raster_weights: 4 per weight, 2 + 3 to renormalise, 3 divisions, 2 additions
    and 1 division for zp), the subtraction from d_h and expf / log1pf in float64 and carries, operation by operation, a bound on
    what float32 can differ by: 2^-24 of the result per rounding plus the propagated operand bounds (class E of
    tests/ordinal_depth_ref.py), 2 ulp = 2^-22 relative for each of expf and log1pf (documented: 1).  So
      |depth - d_o|   <= d_err                  (chore_sil_depth's image against float64, at every winner pixel)
      |coef - coef64| <= coef_err               (sigmoid = 1 / (1 + expf(-x)): 1 expf, 1 addition, 1 division on top of x)
      |sum - sum64|   <= 2^-23 (L + 1) sum|terms| + sum term_err,  L = 16 + ceil(ceil(S^2 / 256) / 256) = 17 for S <= 256, the
                      longest addition chain include/chore_hip.h states (2^-23 (L + 1): gamma_L = L u / (1 - L u) with u = 2^-24,
                      generously).
    The yes / no decisions are the float32 ones on chore_sil_depth's depths (test 1 pins them to chore_render_fwd's).
    The depth rule is ill-conditioned on small and edge-on faces (the determinant of three pixel coordinates of size S cancels
    down to the face's area), and the running bound follows every rounding as if independent: it reaches 1e-3 and more, and is
    infinite on a face whose determinant may vanish.  So coef and the sums are asserted twice: against the whole chain in
    float64 with those bounds, and against the same expressions evaluated on the given float32 depths, where only the
    subtraction, expf, log1pf, one addition and one division round (bounds below 1e-6, asserted finite)."""
    c = scene(B, S, kind)
    ref = c["ref"]
    L = odr.sum_chain(S)
    assert L == 17
    runs = [[x.cpu().numpy() for x in _fwd(c)] for _ in range(2)]
    (sums, coef, counts), again = runs
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0], again)), "two calls differ"
    print("B %d S %d %s: counts %s (reference %s), ties %d, beyond c %d" % (B, S, kind, counts.tolist(), ref["counts"].tolist(),
                                                                              int(ref["tie"].sum()), int(ref["beyond"].sum())))
    print("  depth against float64: largest |error| / bound %.3e (median bound %.3e)"
          % (ref["depth_ratio"], float(np.median(ref["d_err"][ref["d_err"] > 0]))))
    assert ref["depth_ratio"] <= 1
    assert np.array_equal(counts.astype(np.int64), ref["counts"])
    assert ref["tie"][0].sum() > 0 and ref["counts"][0, :2].sum() > 0
    if B > 1:
        assert ref["beyond"][1].sum() > 0 and ref["counts"][2].sum() == 0
    for sfx, what in (("", "whole chain in float64"), ("_g", "on the given float32 depths")):
        cerr = np.abs(coef.astype(np.float64) - ref["coef" + sfx])
        cb = ref["coef_err" + sfx]
        with np.errstate(all="ignore"):
            print("  coef, %s: largest |error| / bound %.3e, largest bound %.3e" % (what, float(np.nanmax(np.where(cb > 0, cerr / cb, 0))),
                                                                                   float(cb.max())))
        assert np.isfinite(coef).all() and (cerr <= cb).all()
        serr = np.abs(sums.astype(np.float64) - ref["sums" + sfx])
        sbound = 2.0 ** -23 * (L + 1) * ref["abs_sums" + sfx] + ref["term_err_sums" + sfx]
        print("  sums, %s: %s, |error| %s, bound %s" % (what, sums, serr, sbound))
        assert (serr <= sbound).all()
    assert np.isfinite(ref["coef_err_g"]).all() and np.isfinite(ref["term_err_sums_g"]).all() and ref["coef_err_g"].max() < 1e-6
    assert (coef[(ref["coef"] == 0)] == 0).all()


@pytest.mark.parametrize("B,S,kind", CASES)
def test_backward_against_float64(B, S, kind):
    """3: grad_tri within the restatement's running bound (the depth rule of chore_render_bwd in float64 on the kernel's own
    coef; a face's sums along a chain of at most (pixels it won) + 9 float32 additions, then one division or three products --
    tests/ordinal_depth_ref.py backward); whether the bits equal chore_render_bwd fed coef * g as grad_depth is printed; a frame
    without a violating pixel and a frame whose every difference exceeds c get exact zeros; the autograd function gives the
    bits of the direct calls"""
    from chore_amd import _lib
    from chore_amd.recon.obj_pose_roi import _OrdinalDepthFn
    c = scene(B, S, kind)
    sil, tri, fim = c["sil"], c["tri"], c["fim"]
    _, coef, _ = _fwd(c)
    g_h = np.array([1.5, -0.75, 2.0][:B], np.float32)
    g = dev(g_h)
    got = _bwd(c, coef, g)
    assert torch.equal(got, _bwd(c, coef, g)), "two calls differ"
    val, err = odr.backward(c["tri_h"], c["fim_h"], coef.cpu().numpy(), g_h)
    d = np.abs(got.cpu().numpy().astype(np.float64) - val)
    with np.errstate(all="ignore"):
        print("B %d S %d %s: backward, largest |error| / bound %.3e, largest entry %.3e"
              % (B, S, kind, float(np.nanmax(np.where(err > 0, d / err, 0))), float(np.abs(val).max())))
    assert np.isfinite(got.cpu().numpy()).all() and (d <= err).all() and np.abs(val[0]).max() > 0
    if B > 1:
        assert not got[1].any() and not got[2].any()
        assert (coef[1] == 0).all() and c["ref"]["beyond"][1].sum() > 0
    # chore_render_bwd with this gradient as grad_depth alone
    h = _lib.handle(0)
    Fn = tri.shape[1]
    tex = torch.zeros(B, Fn, 2, 2, 2, 3, device="cuda")
    gd = (coef * g.view(-1, 1, 1)).contiguous()
    want = torch.empty_like(got)
    ws = torch.empty(_lib.lib.chore_render_bwd_workspace_bytes(B, Fn, 2, S, 1), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.chore_render_bwd(h, tri.data_ptr(), tex.data_ptr(), None, fim.data_ptr(), B, Fn, 2, S, 1, NEAR, FAR, 1e-3, 1e-3,
                                         (ctypes.c_float * 3)(0, 0, 0), None, gd.data_ptr(), None, want.data_ptr(), None, None,
                                         ws.data_ptr(), _stream()), h, "chore_render_bwd")
    print("  bits equal chore_render_bwd's: %s (largest difference %.3e)" % (torch.equal(got, want), float((got - want).abs().max())))
    leaf = tri.clone().requires_grad_(True)
    out = _OrdinalDepthFn.apply(leaf, fim, sil.occ_depth, sil.image_ref, sil.keep_mask, odr.C)
    out.backward(g)
    assert torch.equal(out.detach(), _fwd(c)[0]) and torch.equal(leaf.grad, got)


@pytest.mark.parametrize("mirrored", [False, True])
def test_sign_and_use(mirrored):
    """4: a box in front of the body under a person-labelled view: depth > 0, d loss / d obj_t[z] < 0, and 20 Adam steps on
    obj_t lower the case-A count; mirrored (the box behind the body, an object-labelled view): the gradient is > 0 and the steps
    lower the case-B count"""
    from chore_amd.recon.obj_pose_roi import SilLossROI
    S = 64
    body, bfaces = _body()
    body = body[:1]
    ov, of = odr.box_verts(), odr.BOX_FACES
    ref = np.full((1, S, S), mirrored)
    sil = SilLossROI.from_crops(ref, ~ref, _roi_K(body), ov, of)
    sil.set_occluder(dev(body), bfaces)
    occ = sil.occ_depth
    assert (occ < FAR).sum() > 200
    R = dev(odr.rot_xyz(0.3, 0.2, 0.1)[None])
    s = torch.ones(1).cuda()
    mid = occ[0, S // 4: 3 * S // 4, S // 4: 3 * S // 4]        # the body's surface in the middle of the view, where the box is
    near_z = float(mid[mid < FAR].min()) if not mirrored else float(mid[mid < FAR].max())
    c = _centre(body[0])
    t0z = near_z + (0.2 if mirrored else -0.2)
    t = dev(np.array([[c[0], c[1], t0z]], np.float32)).requires_grad_(True)
    col = 1 if mirrored else 0

    def loss_and_counts():
        _, tri, fim = sil.render_parts(R, t, s)
        return sil.depth_loss(tri, fim)["depth"], sil.depth_order_counts(R, t.detach(), s)[0].tolist()
    loss, counts0 = loss_and_counts()
    loss.backward()
    loss0 = float(loss.detach())
    gz = float(t.grad[0, 2])
    print("mirrored %s: depth %.4f, d depth / d t_z %.4f, counts %s" % (mirrored, loss0, gz, counts0))
    assert loss0 > 0 and counts0[col] > 20 and counts0[1 - col] == 0
    assert gz > 0 if mirrored else gz < 0
    opt = torch.optim.Adam([t], lr=0.06)
    for _ in range(20):
        opt.zero_grad()
        loss, _ = loss_and_counts()
        loss.backward()
        opt.step()
    loss1, counts1 = loss_and_counts()
    print("  after 20 Adam steps: depth %.4f, t_z %.3f -> %.3f, counts %s" % (float(loss1.detach()), t0z, float(t[0, 2].detach()), counts1))
    assert counts1[col] < counts0[col] and float(loss1.detach()) < loss0


# ---- 5. fitter -------------------------------------------------------------------------------------------------------------
def _fit_objects(opt, net=None, flip=False, on=True):
    from test_gpu_sil_targets import _fit_objects as base
    fitter, net, data = base(opt, net=net, flip=flip)
    fitter.ORDINAL_DEPTH_TERM = on
    return fitter, net, data


def _run(fitter, net, data, log=None, joint_iter=0):
    if log is not None:
        orig = fitter.forward_step

        def f(*a, **k):
            ld = orig(*a, **k)
            log.append((a[6] if len(a) > 6 else k["phase"], {k_: v.detach() for k_, v in ld.items()}))
            return ld
        fitter.forward_step = f
    torch.manual_seed(12)
    data["smpl_fitted"], R, t = fitter.optimize_smpl_object(net, data, obj_iter=1, joint_iter=joint_iter, steps_per_iter=3, sil_iter=2, max_iter=0)
    return [x.detach().clone() for x in (R, t, data["obj_s"])]


def test_fitter_with_the_ordinal_depth_term(opt, tmp_path):
    """5: ORDINAL_DEPTH_TERM = True (B = 2, S = 64).  A short 'object only' + 'sil' + 'joint' schedule: a finite "depth", last
    key, in every 'sil' and 'joint' step and > 0 in each phase; the recorded fit of that schedule has R bit-equal to the eager
    one (R is not stepped in 'joint') and t, s within 2e-4, the Adam round-off bound tests/test_gpu_fit_chain.py
    (test_graph_replay_follows_the_same_schedule) holds the same comparison to -- a 'joint' iteration is not bit-equal between
    eager and recorded steps with the switch off either (measured in two runs, t / s: up to 2.9e-5 / 2.2e-5 off, 5.4e-5 / 5.3e-5
    on; both printed).
    The schedule of test_fitter_with_device_setup_and_edge_term ('object only' + 'sil'): eager and recorded fits bit-equal; a
    second batch through the kept slot (masks by set_masks, occluder by set_occluder, both in place) bit-equal to a fresh
    fitter.  The report file holds the counts the kept term's kernel gives at the fitted pose, and they are not all zero."""
    from chore_amd.recon.obj_pose_roi import SilLossROI
    log = []
    eager, net, data = _fit_objects(opt)
    res_joint = _run(eager, net, data, log, joint_iter=1)
    for phase in ("sil", "joint"):
        steps = [ld for p, ld in log if p == phase]
        assert len(steps) >= 3 and all(list(ld)[-1] == "depth" for ld in steps), phase
        depth = torch.stack([ld["depth"] for ld in steps])
        print("depth term per '%s' step: %s" % (phase, depth.tolist()))
        assert torch.isfinite(depth).all() and (depth >= 0).all() and float(depth.max()) > 0
    assert all("depth" not in ld for p, ld in log if p == "object only")
    for on in (True, False):
        res_e = res_joint
        if not on:
            e_, _, d_ = _fit_objects(opt, net=net, on=False)
            res_e = _run(e_, net, d_, joint_iter=1)
        g_, _, d_ = _fit_objects(opt, net=net, on=on)
        g_.use_graphs = True
        res_g = _run(g_, net, d_, joint_iter=1)
        diffs = [float((a - b).abs().max()) for a, b in zip(res_e, res_g)]
        print("with a 'joint' iteration, switch %s: eager vs graph, largest difference of R, t, s: %s" % ("on" if on else "off", diffs))
        assert all(torch.isfinite(x).all() for x in res_g)
        assert torch.equal(res_e[0], res_g[0]) and diffs[1] < 2e-4 and diffs[2] < 2e-4, (on, diffs)
    assert not torch.equal(res_e[1], res_joint[1])              # the term does move the fit
    eager, _, data = _fit_objects(opt, net=net)
    res_eager = _run(eager, net, data)
    sil = data["silhouette"]
    assert isinstance(sil, SilLossROI) and tuple(sil.occ_depth.shape) == (2, 64, 64)
    print("occluder: %d of %d pixels see the body" % (int((sil.occ_depth < FAR).sum()), sil.occ_depth.numel()))
    assert float(eager.get_loss_weights()["depth"](1.0, 0)) == float(eager.get_loss_weights()["mask"](1.0, 0)) == 0.003 ** 2
    graphed, _, data = _fit_objects(opt, net=net)
    graphed.use_graphs = True
    res_graph = _run(graphed, net, data)
    for name, a, b in zip(("R", "t", "s"), res_eager, res_graph):
        print("eager vs graph %s: largest difference %.3e" % (name, float((a - b).abs().max())))
    for name, a, b in zip(("R", "t", "s"), res_eager, res_graph):
        assert torch.isfinite(b).all() and torch.equal(a, b), name
    keeper, _, data = _fit_objects(opt, net=net)
    keeper.use_graphs = keeper.reuse_graphs = True
    first = _run(keeper, net, data)
    kept_sil = data["silhouette"]
    kept_ptr = kept_sil.occ_depth.data_ptr()
    for a, b in zip(first, res_graph):
        assert torch.equal(a, b)
    _, _, data2 = _fit_objects(opt, net=net, flip=True)
    second = _run(keeper, net, data2)
    assert data2["silhouette"] is kept_sil and len(keeper._slots) == 1 and kept_sil.occ_depth.data_ptr() == kept_ptr
    fresh, _, data3 = _fit_objects(opt, net=net, flip=True)
    fresh.use_graphs = True
    want = _run(fresh, net, data3)
    for name, a, b in zip(("R", "t", "s"), second, want):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    for n in ("image_ref", "keep_mask", "K", "occ_depth"):
        assert torch.equal(getattr(kept_sil, n), getattr(data3["silhouette"], n)), n
    # the report: save_outputs (which builds a term of its own from the batch's masks and the written meshes) against the counts
    # the fit's own term -- its masks by set_masks, its occluder by set_occluder -- gives at the fitted pose
    fresh.REPORT_DEPTH_ORDER = True
    fresh.outpath = str(tmp_path)
    paths = [os.path.join("seq", "t%04d" % i, "k1.color.jpg") for i in range(2)]
    fresh.save_outputs(data3["smpl_fitted"], want[0], want[1], paths, "fit", 1, want[2], images=data3["images"],
                       crop_centers=data3["query_dict"]["crop_center"])
    counts = kept_sil.depth_order_counts(fresh.decopose_axis(want[0], no_rand=True), want[1], want[2]).tolist()
    assert sum(c[2] + c[3] for c in counts) > 0 and sum(c[0] + c[1] for c in counts) > 0
    for i in range(2):
        rep = json.load(open(os.path.join(str(tmp_path), "seq", "t%04d" % i, "fit", "k1.depth_order.json")))
        print("frame %d report: %s" % (i, rep))
        assert [rep[k] for k in ("person_pixels_object_in_front", "object_pixels_body_in_front", "person_pixels_both",
                                 "object_pixels_both")] == counts[i]
        assert rep["person_violated_fraction"] == (counts[i][0] / counts[i][2] if counts[i][2] else None)
        assert rep["object_violated_fraction"] == (counts[i][1] / counts[i][3] if counts[i][3] else None)


def test_the_switch_is_off_by_default(opt):
    """5 (off): False by default; then no "depth" key and no occ_depth buffer; the two settings keep their recorded steps under
    different slot keys"""
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    from chore_amd.recon.recon_fit_coco import ReconFitterCoco
    assert ReconFitterBase.ORDINAL_DEPTH_TERM is False and ReconFitterBase.REPORT_DEPTH_ORDER is False
    f = ReconFitterCoco.from_parts(device="cuda:0")
    assert "depth" not in f.get_loss_weights()
    f.ORDINAL_DEPTH_TERM = True
    assert float(f.get_loss_weights()["depth"](1.0, 0)) == float(f.get_loss_weights()["mask"](1.0, 0))
    log = []
    off, net, data = _fit_objects(opt, on=False)
    off.use_graphs = off.reuse_graphs = True
    res_off = _run(off, net, data, log)
    assert all("depth" not in ld for _, ld in log) and not hasattr(data["silhouette"], "occ_depth")
    on, _, data_on = _fit_objects(opt, net=net)
    on.use_graphs = on.reuse_graphs = True
    on._slots = off._slots                      # one table of kept slots: the two settings must not share an entry
    res_on = _run(on, net, data_on)
    assert len(off._slots) == 2 and {k[-1] for k in off._slots} == {False, True}
    print("switch off vs on, largest difference of t: %.3e" % float((res_off[1] - res_on[1]).abs().max()))


def test_refuses_what_it_cannot_do():
    """CHORE_EINVAL, before anything is launched, for NULL pointers and for shapes the calls do not take; 0 workspace bytes"""
    from chore_amd import _lib
    L, h = _lib.lib, _lib.handle(0)
    x = torch.zeros(4096, device="cuda")
    xi = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p, q, st = x.data_ptr(), xi.data_ptr(), _stream()
    EINVAL = L.chore_sil_depth(h, None, q, 1, 1, 8, FAR, 1, p, st)
    assert EINVAL != 0 and EINVAL == L.chore_sil_depth(h, p, None, 1, 1, 8, FAR, 1, p, st) == L.chore_sil_depth(h, p, q, 1, 1, 8, FAR, 1, None, st)
    for B, F, S in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (1, 1, 4097), (65536, 1, 8)):
        assert L.chore_sil_depth(h, p, q, B, F, S, FAR, 1, p, st) == EINVAL
        assert L.chore_ordinal_depth_fwd(h, p, q, p, p, p, B, F, S, FAR, 2.0, p, p, q, p, st) == EINVAL
        assert L.chore_ordinal_depth_bwd(h, p, q, p, p, B, F, S, p, st) == EINVAL
        if (B, F, S) != (1, 0, 8):
            assert L.chore_ordinal_depth_workspace_bytes(B, S) == 0
    for c in (0.0, -1.0, float("nan"), 81.0):
        assert L.chore_ordinal_depth_fwd(h, p, q, p, p, p, 1, 1, 8, FAR, c, p, p, q, p, st) == EINVAL
    args = [p, q, p, p, p]
    for i in range(5):
        a = list(args)
        a[i] = None
        assert L.chore_ordinal_depth_fwd(h, *a, 1, 1, 8, FAR, 2.0, p, p, q, p, st) == EINVAL
    for i in range(4):
        a = [p, q, p, p]
        a[i] = None
        assert L.chore_ordinal_depth_bwd(h, *a, 1, 1, 8, p, st) == EINVAL
    assert L.chore_ordinal_depth_bwd(h, p, q, p, p, 1, 1, 8, None, st) == EINVAL
    assert L.chore_ordinal_depth_fwd(h, p, q, p, p, p, 1, 1, 8, FAR, 2.0, p, p, q, None, st) == EINVAL
    assert L.chore_ordinal_depth_workspace_bytes(3, 40) >= 4 * 3 * 7 * 5 and L.chore_ordinal_depth_workspace_bytes(3, 40) % 256 == 0
    torch.cuda.synchronize()
