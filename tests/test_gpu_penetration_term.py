"""GPU: the opt-in interpenetration term (recon/eval/penetration.py penetration_loss, ReconFitterBase.compute_penetration_loss,
PENETRATION_TERM) on top of the differentiable mesh distance: its value is what the penetration report prints, its gradient
is checked against the float64 restatement (tests/mesh_grad_ref.py), it separates two spheres, and the joint phase runs with
it eagerly and as recorded graphs."""
import numpy as np
import pytest
import torch

import mesh_grad_ref as gref
import mesh_sign_ref as sref
from mesh_grad_ref import f32
from meshes import icosphere

pytestmark = pytest.mark.gpu


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def test_loss_is_the_report():
    """1: penetration_loss = frac * mean_depth of penetration(), rtol 1e-6 (three fp32 roundings), both directions, B = 2"""
    from chore_amd.recon.eval.penetration import penetration, penetration_loss
    VA, FA, VB, FB = gref.sphere_pair()
    va = dev(np.stack([VA, f32(VA + np.array([0.05, 0.0, 0.0]))]), np.float32)
    vb = dev(np.stack([VB, f32(VB + np.array([5.0, 0.0, 0.0]))]), np.float32)           # frame 1: apart
    for a, fa, b in ((va, FA, vb), (vb, FB, va)):
        loss = penetration_loss(a, dev(fa, np.int32), b)
        rep = penetration(a, dev(fa, np.int32), b)
        want = rep["frac"] * rep["mean_depth"]
        print("penetration_loss %s  frac * mean_depth %s  count %s" % (loss.tolist(), want.tolist(), rep["count"].tolist()))
        assert tuple(loss.shape) == (2,) and loss.dtype == torch.float32 and not loss.requires_grad
        assert float(loss[0]) > 0 and float(loss[1]) == 0 and int(rep["count"][1]) == 0
        assert torch.allclose(loss, want, rtol=1e-6, atol=0)
    one = penetration_loss(va[0], dev(FA, np.int32), vb[0])                              # unbatched
    assert tuple(one.shape) == (1,) and torch.equal(one, penetration_loss(va, dev(FA, np.int32), vb)[:1])


def test_descent_separates_two_spheres():
    """2: steps of 0.05 m along the negative normalized gradient of pen(A,B) + pen(B,A) with respect to the small sphere's
    translation: strictly decreasing, exactly 0 with zero gradient within 8 steps, the step-0 gradient along the centre line
    (cosine >= 0.99) and within 8 x E32 of float64, and the report counts 0 at the end"""
    from chore_amd.recon.eval.penetration import penetration, penetration_loss
    VA, FA, VB, FB = gref.sphere_pair()
    va, vb0, fa, fb = dev(VA, np.float32), dev(VB, np.float32), dev(FA, np.int32), dev(FB, np.int32)
    l64, g64, cnt = gref.pair_loss(VA, FA, VB, FB)
    g32 = gref.pair_loss(VA, FA, VB, FB, np.float32)[1]
    E32 = float(np.abs(g32 - g64).max())
    t = torch.zeros(3, device="cuda", requires_grad=True)
    losses = []
    for step in range(9):
        vb = vb0 + t
        loss = (penetration_loss(va, fa, vb) + penetration_loss(vb, fb, va))[0]
        grad, = torch.autograd.grad(loss, t)
        losses.append(float(loss.detach()))
        if step == 0:
            g = grad.cpu().numpy().astype(np.float64)
            line = np.array([1.13, 0.21, 2.37]) - np.array([0.0, 0.0, 2.2])
            cos = -(g @ line) / (np.linalg.norm(g) * np.linalg.norm(line))
            err = np.abs(g - g64).max()
            print("step 0: loss %.6f (float64 %.6f, inside %s)  gradient %s  float64 %s  |diff| %.3e  E32 %.3e  cosine %.5f"
                  % (losses[0], l64, cnt, g, g64, err, E32, cos))
            assert 0 < E32 < 1e-2 and err <= 8 * E32 and cos >= 0.99
            assert abs(losses[0] - l64) <= 1e-6
        if losses[-1] == 0:
            assert not grad.any()
            break
        with torch.no_grad():
            t -= 0.05 * grad / grad.norm()
    print("loss per step:", ["%.4f" % x for x in losses])
    assert losses[-1] == 0 and len(losses) <= 9                      # the 9th evaluation is the state after 8 steps
    assert all(b < a for a, b in zip(losses, losses[1:]))
    vb = (vb0 + t).detach()
    assert int(penetration(va, fa, vb)["count"][0]) == 0 and int(penetration(vb, fb, va)["count"][0]) == 0


def _fitter(scan_v, scan_f):
    from chore_amd.recon.recon_fit_behave import ReconFitterBehave
    return ReconFitterBehave.from_parts(device="cuda:0", scan_verts=scan_v, scan_faces=scan_f)


def test_compute_penetration_loss_and_the_open_template():
    """3 (the term itself): both directions for a closed template, the one direction for an open one (hemisphere); the value
    is the report's; finite, non-zero gradient on the translation of a pose that penetrates"""
    from chore_amd.recon.eval.penetration import penetration_loss
    VA, FA = icosphere(3, 1.0)
    body_v, body_f = dev(f32(VA)[None].repeat(2, 0), np.float32), dev(FA, np.int64)
    R = torch.eye(3).cuda()[None].repeat(2, 1, 1)
    s = torch.ones(2).cuda()
    Vc, Fc = icosphere(2, 0.5)
    Vh, Fh = sref.hemisphere(2, 0.5)
    for V, F, closed in ((Vc, Fc, True), (Vh, Fh, False)):
        fitter = _fitter(f32(V), F)
        assert fitter.PENETRATION_TERM is False
        t = torch.tensor([[1.13, 0.21, 0.17], [5.0, 0.0, 0.0]]).cuda().requires_grad_(True)      # frame 1: apart
        loss = fitter.compute_penetration_loss(body_v, body_f, R, t, s)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and float(loss) > 0
        obj = dev(f32(V)[None], np.float32) + t.detach()[:, None, :]
        want = penetration_loss(body_v, body_f, obj)
        both = want + penetration_loss(obj, dev(F, np.int64), body_v)
        assert float(want[0]) > 0 and float(both[1]) == 0
        if closed:
            assert float(both[0]) > float(want[0])
        assert torch.allclose(loss, (both if closed else want).mean(), rtol=1e-6, atol=0), closed
        rep = fitter.penetration_report(body_v, body_f, R, t, s)
        assert (rep["body_in_object"] is not None) == closed
        total = rep["object_in_body"]["frac"] * rep["object_in_body"]["mean_depth"]
        if closed:
            total = total + rep["body_in_object"]["frac"] * rep["body_in_object"]["mean_depth"]
        assert torch.allclose(loss, total.mean(), rtol=1e-5, atol=0)
        loss.backward()
        assert torch.isfinite(t.grad).all() and float(t.grad[0].abs().max()) > 0 and float(t.grad[1].abs().max()) == 0
        assert float(t.grad[0, 0]) < 0                               # moving the object away from the body (+x) lowers the term


def _fit_objects(opt, net=None, B=2):
    """a rigid closed body with SMPL's counts, the template of tests/fit_harness.py and a pose that penetrates
    (also the synthetic fit of scripts/mesh_dist_bwd_bench.py)"""
    import copy
    from chore_amd.lib_smpl.priors import synthetic_priors
    from chore_amd.lib_smpl.wrapper_pytorch import SMPLPyTorchWrapperBatch
    from chore_amd.model import CHORE
    from chore_amd.recon.recon_fit_behave import ReconFitterBehave
    from chore_amd.utils import synth
    from fit_harness import template_mesh
    from meshes import uv_ellipsoid
    from test_gpu_query import nhwc
    rs = np.random.RandomState(9)
    if net is None:
        opt = copy.copy(opt)
        opt.compute_dtype = "fp32"
        net = CHORE(opt).cuda().eval()
        synth.load_synth_weights(net, seed=0)
        for p in net.parameters():
            p.requires_grad_(False)
        net.im_feat_list = [nhwc((rs.standard_normal((B, 256, 32, 32)) * 0.5).astype(np.float32))]
        net.tmpx = nhwc((rs.standard_normal((B, 64, 64, 64)) * 0.5).astype(np.float32))
    else:
        rs.standard_normal((B, 256, 32, 32)), rs.standard_normal((B, 64, 64, 64))       # the same draws after it
    body_v, body_f = uv_ellipsoid()
    model = synth.synth_smplh_model(0)
    model["v_template"] = body_v.astype(np.float32)
    model["shapedirs"] = np.zeros_like(model["shapedirs"])
    model["posedirs"] = np.zeros_like(model["posedirs"])
    trans = np.array([[0.0, 0.3, 2.2], [0.05, 0.25, 2.3]], np.float32)[np.arange(B) % 2]
    smpl = SMPLPyTorchWrapperBatch(model, B, betas=torch.zeros(B, 10), pose=torch.zeros(B, 156), trans=torch.from_numpy(trans),
                                   faces=torch.from_numpy(body_f)).cuda()
    obj_v, obj_f = template_mesh()
    body_prior, hand_prior = synthetic_priors(0)
    labels = torch.from_numpy(rs.randint(0, 14, 6890)).cuda()
    fitter = ReconFitterBehave.from_parts(device="cuda:0", part_labels=labels, body_prior=body_prior, hand_prior=hand_prior,
                                          scan_verts=obj_v, scan_faces=obj_f)
    fitter.adam_capturable = True
    cc = torch.tensor([synth.CROP_CENTER] * B).cuda()
    obj = torch.from_numpy(np.stack([obj_v[rs.randint(0, len(obj_v), 3000)]] * B).astype(np.float32)).cuda()
    t0 = trans + np.array([0.3, 0.1, 0.02], np.float32)
    data = dict(net=net, query_dict={"crop_center": cc}, part_labels=labels.unsqueeze(0).repeat(B, 1), objects=obj, smpl=smpl,
                obj_R=torch.eye(3).repeat(B, 1, 1).cuda().requires_grad_(True),
                obj_t=torch.from_numpy(t0).cuda().requires_grad_(True), obj_s=torch.ones(B).cuda().requires_grad_(True))
    return fitter, net, smpl, data


def _run(fitter, net, data):
    torch.manual_seed(11)
    _, R, t = fitter.optimize_smpl_object(net, data, obj_iter=2, joint_iter=2, steps_per_iter=5, max_iter=1, sil_iter=0)
    return [x.detach().clone() for x in (R, t, data["obj_s"])]


def test_forward_step_switch(opt):
    """3 (the fitter): switch off, forward_step(..., 'joint') has no 'pen' key; switch on, the key is a 0-d float32 device tensor
    equal to compute_penetration_loss, and the weighted sum's backward gives finite, non-zero obj_t.grad"""
    fitter, net, smpl, data = _fit_objects(opt)
    B = 2
    split = fitter.split_smpl(smpl)
    data["smpl_center"] = fitter.compute_smpl_center_pred(data, net, smpl)
    noise = torch.zeros(B, 3, 3).cuda()
    off = fitter.forward_step(net, split, data, data["obj_R"], data["obj_t"], data["obj_s"], "joint", noise=noise)
    assert "pen" not in off and "collide" in off
    fitter.PENETRATION_TERM = True
    assert "pen" not in fitter.forward_step(net, split, data, data["obj_R"], data["obj_t"], data["obj_s"], "object only", noise=noise)
    on = fitter.forward_step(net, split, data, data["obj_R"], data["obj_t"], data["obj_s"], "joint", noise=noise)
    assert list(on)[-2:] == ["collide", "pen"] and [k for k in on if k != "pen"] == list(off)
    pen = on["pen"]
    assert pen.dim() == 0 and pen.dtype == torch.float32 and pen.is_cuda and float(pen) > 0
    R = fitter.decopose_axis(data["obj_R"], noise=noise)
    want = fitter.compute_penetration_loss(split()[0], split.faces, R, data["obj_t"], data["obj_s"])
    assert torch.equal(pen.detach(), want.detach())
    for k in off:
        assert torch.equal(off[k].detach(), on[k].detach()), k        # the other terms do not change
    wd = fitter.get_loss_weights()
    assert float(wd["pen"](1.0, 0)) == 900.0
    # the term alone, then the whole sum
    g_pen, = torch.autograd.grad(pen, data["obj_t"], retain_graph=True)
    assert torch.isfinite(g_pen).all() and float(g_pen.abs().max()) > 0
    fitter.sum_dict(on, wd, 1).backward()
    g = data["obj_t"].grad
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    del on, off, pen, want
    fitter.release_graphs(split, net)()


def test_joint_phase_with_the_term(opt):
    """4: a short optimize_smpl_object with the term on: recorded graphs against eager within 1e-5; the term moves the fit;
    with reuse_graphs a call with the switch off after one with it on returns the switch-off result of a fresh fitter bit for
    bit (the switch is part of the slot key)"""
    res = {}
    for graphs in (False, True):
        fitter, net, smpl, data = _fit_objects(opt)
        fitter.use_graphs, fitter.PENETRATION_TERM = graphs, True
        res[graphs] = _run(fitter, net, data)
    for name, a, b in zip(("R", "t", "s"), res[False], res[True]):
        assert torch.isfinite(b).all(), name
        assert float((a - b).abs().max()) < 1e-5, (name, float((a - b).abs().max()))
    fresh, net, smpl, data = _fit_objects(opt)
    fresh.use_graphs = fresh.reuse_graphs = True
    off_fresh = _run(fresh, net, data)
    assert float((off_fresh[1] - res[True][1]).abs().max()) > 1e-6                     # the term does change the fit
    keeper, net, smpl, data = _fit_objects(opt)
    keeper.use_graphs = keeper.reuse_graphs = True
    keeper.PENETRATION_TERM = True
    on_kept = _run(keeper, net, data)
    for a, b in zip(on_kept, res[True]):
        assert torch.equal(a, b)
    keeper.PENETRATION_TERM = False
    _, _, smpl, data = _fit_objects(opt, net=net)
    off_kept = _run(keeper, net, data)
    assert len(keeper._slots) == 2                                                     # one slot per setting of the switch
    for name, a, b in zip(("R", "t", "s"), off_fresh, off_kept):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
