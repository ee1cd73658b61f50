"""GPU parity tests of the stacked-hourglass encoder (chore_encode_fwd) against the reference's
outputs (tests/golden/encoder_*.npz) and the numpy oracle.

Stated tolerances
  fp32 mode (exact-fp32 MFMA):  max |err| <= 2e-4 * max|ref| per tensor (150 layers, different
                                summation order than MKL/oneDNN).
  bf16 mode (bf16 storage + bf16 MFMA operands, fp32 accumulate and GroupNorm statistics):
                                relative L2 error <= 2e-2 per tensor, max |err| <= 8e-2 * max|ref|.
"""
import os

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import encoder as oe

pytestmark = pytest.mark.gpu


def make_net(opt, dtype):
    from chore_amd.model import CHORE
    from chore_amd.utils import synth
    opt.compute_dtype = dtype
    m = CHORE(opt).cuda().eval()
    synth.load_synth_weights(m, seed=0)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def rel_max(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def rel_l2(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


@pytest.fixture(scope="module")
def net32(opt):
    return make_net(opt, "fp32")


@pytest.fixture(scope="module")
def net16(opt):
    return make_net(opt, "bf16")


def encode(net, images, train):
    net.train(train)
    try:
        with torch.no_grad():
            net.filter(torch.from_numpy(images).cuda())
    finally:
        net.train(False)
    outs = [o.float().cpu().numpy() for o in net.im_feat_list]
    return outs, net.tmpx.float().cpu().numpy(), net.normx.float().cpu().numpy()


def test_encoder_fp32_matches_reference(net32, synth_sd):
    g = golden("encoder_64x96.npz")
    outs, tmpx, normx = encode(net32, g["images"], train=True)
    assert len(outs) == 5 and outs[-1].shape == (1, 256, 16, 24) and tmpx.shape == (1, 64, 32, 48)
    # feature maps are NHWC in memory behind the (B,C,H,W) view
    assert net32.tmpx.stride() == (32 * 48 * 64, 1, 48 * 64, 64)
    assert rel_max(tmpx, g["tmpx"]) < 2e-5
    assert rel_max(normx, g["normx"]) < 1e-4
    assert rel_max(outs[-1], g["out_last"]) < 2e-4
    assert rel_max(outs[0][:, :, 4:8, 8:12], g["out_first_crop"]) < 2e-4
    np.testing.assert_allclose(np.stack([o.mean((0, 2, 3)) for o in outs]), g["out_means"], rtol=1e-3, atol=1e-3)
    # and the oracle agrees stage by stage
    o_outs, o_tmpx, o_normx = oe.Encoder(synth_sd).forward(g["images"])
    for a, b in zip(outs, o_outs):
        assert rel_max(a, b) < 2e-4
    # eval mode keeps only the last stack and gives the same tensor -- to fp32 round-off: the outputs of stacks 0-3 are
    # not produced there, and their l / bl / al 1x1 convolutions run merged into one (W_bl + W_al W_l, composed in fp64)
    outs_e, _, _ = encode(net32, g["images"], train=False)
    assert len(outs_e) == 1 and rel_max(outs_e[0], outs[-1]) < 2e-5
    assert rel_max(outs_e[0], g["out_last"]) < 2e-4


def test_encoder_bf16_within_stated_tolerance(net16):
    g = golden("encoder_64x96.npz")
    outs, tmpx, normx = encode(net16, g["images"], train=True)
    assert net16.tmpx.dtype == torch.bfloat16
    for name, a, b in (("tmpx", tmpx, g["tmpx"]), ("normx", normx, g["normx"]), ("out_last", outs[-1], g["out_last"])):
        assert rel_l2(a, b) < 2e-2, (name, rel_l2(a, b))
        assert rel_max(a, b) < 8e-2, (name, rel_max(a, b))


def test_encoder_fp16_modes_on_a_ragged_shape(opt, net32):
    """64 x 96 image (maps 32 x 48 ... 4 x 6: ragged 32-pixel tiles, maps smaller than a tile) in the two modes that run the
    specialised-wave convolution: fp16x3 (eval, fp32-grade) and fp16 (half feature maps, a 1e-3 mode)"""
    g = golden("encoder_64x96.npz")
    import copy
    for mode, tol_max, tol_l2 in (("fp16x3", 2e-4, 1e-4), ("fp16", 2e-2, 4e-3)):
        net = make_net(copy.copy(opt), mode)
        outs, tmpx, normx = encode(net, g["images"], train=False)
        assert net.tmpx.dtype == (torch.float16 if mode == "fp16" else torch.float32)
        for name, a, b in (("tmpx", tmpx, g["tmpx"]), ("normx", normx, g["normx"]), ("out_last", outs[-1], g["out_last"])):
            assert rel_max(a, b) < tol_max, (mode, name, rel_max(a, b))
            assert rel_l2(a, b) < tol_l2, (mode, name, rel_l2(a, b))


@pytest.mark.parametrize("mode,B", [pytest.param(m, b, id=m if b == 1 else "%s-b%d" % (m, b))
                                    for b in (1, 4) for m in ("fp32", "bf16", "fp16x3", "fp16")])
def test_encoder_512_checksums(request, opt, mode, B):
    """BASELINE size (512x512) against per-channel statistics and crops of the reference output, in every compute mode; B = 4 (the
    benchmark's batch: other tilings, residual epilogues, strided slice outputs and raw copies at production size) stacks the
    golden's image first with three others and compares image 0.  fp16x3 is held to the fp32 bounds, as everywhere in the project;
    fp16 (half maps, three more mantissa bits than bf16) to the bf16 bounds."""
    import copy
    from chore_amd.utils import synth
    net = (request.getfixturevalue("net32") if mode == "fp32" else request.getfixturevalue("net16") if mode == "bf16"
           else make_net(copy.copy(opt), mode))
    g = golden("encoder_512_checksum.npz")
    images = synth.synth_images(1, 512, 512, seed=0)
    if B > 1:
        images = np.concatenate([images, synth.synth_images(B - 1, 512, 512, seed=1)])
    outs, tmpx, _ = encode(net, images, train=False)
    assert outs[0].shape == (B, 256, 128, 128)
    out, tmpx = outs[0][:1], tmpx[:1]
    tol_max, tol_mean = (3e-4, 2e-4) if mode in ("fp32", "fp16x3") else (1e-1, 1e-2)
    assert rel_max(out[:, :, 60:68, 100:108], g["out_crop"]) < tol_max
    assert rel_max(tmpx[:, :, 128:132, 200:204], g["tmpx_crop"]) < tol_max
    s = np.abs(g["out_absmean"]).max()
    assert np.abs(out.mean((0, 2, 3)) - g["out_mean"]).max() < tol_mean * s
    assert np.abs(np.abs(out).mean((0, 2, 3)) - g["out_absmean"]).max() < tol_mean * s


def test_encoder_batch_independence(net32):
    """size-independent property: every image of a batch is encoded independently (GroupNorm is
    per sample), so a batch of 2 different images equals the two single-image runs bit for bit"""
    from chore_amd.utils import synth
    imgs = synth.synth_images(2, 64, 64, seed=5)
    both, tb, _ = encode(net32, imgs, train=False)
    for i in range(2):
        one, t1, _ = encode(net32, imgs[i:i + 1], train=False)
        assert np.array_equal(one[0][0], both[0][i]) and np.array_equal(t1[0], tb[i])


def test_end_to_end_filter_query_matches_oracle(net32, synth_sd):
    """config 1 shape of work at reduced image size: encode + query through the public API"""
    from chore_amd.utils import synth
    from oracle import query as oq
    img = synth.synth_images(1, 128, 128, seed=2)
    pts = synth.synth_points(1, 2048, seed=3)
    cc = np.array([synth.CROP_CENTER], np.float32)
    with torch.no_grad():
        net32.filter(torch.from_numpy(img).cuda())
        net32.query(torch.from_numpy(pts).cuda(), crop_center=torch.from_numpy(cc).cuda())
    df, pca, parts, centers = [t.cpu().numpy() for t in net32.get_preds()]
    outs, tmpx, _ = oe.Encoder(synth_sd).forward(img)
    o = oq.query(pts, cc, outs[-1], tmpx, synth_sd)
    for k, v in dict(df=df, pca=pca, parts=parts, centers=centers).items():
        assert np.abs(v - o[k]).max() < 1e-4 * max(1.0, np.abs(o[k]).max()), k


def test_training_forward_loss_matches_reference(opt):
    """CHORE.forward in training mode = encoder with all 5 stack outputs + 5 field queries + get_errors
    (model/chore.py:176-237): total error and the six averaged loss terms against the reference's
    values (tests/golden/train_loss.npz).  fp32 mode, 1e-4 relative; forward only (the backward to the network
    parameters is not built: the parameters are frozen and the loss is evaluated under no_grad)."""
    import copy
    g = golden("train_loss.npz")
    net = make_net(copy.copy(opt), "fp32")
    net.train(True)
    keys = ("images", "points", "df_h", "df_o", "parts_gt", "pca_gt", "body_center", "obj_center", "crop_center")
    with torch.no_grad():
        error, losses_all = net.forward(**{k: torch.from_numpy(g[k]).cuda() for k in keys})
    assert len(net.intermediate_preds_list) == 5
    np.testing.assert_allclose(net.intermediate_preds_list[0][0][:, :, :64].cpu().numpy(), g["df_stack0"], atol=2e-5)
    np.testing.assert_allclose(losses_all.numpy(), g["losses_all"], rtol=1e-4)
    assert abs(float(error) - float(g["error"])) < 1e-4 * abs(float(g["error"]))
    assert set(net.format_sep_losses(losses_all)) == {"df_h", "df_o", "parts", "pca", "smpl", "obj"}


def test_heads_train_on_a_frozen_encoder(opt):
    """CHORE.forward + backward + Adam on the 32 head parameters with the encoder frozen (the part of the training
    step that is built): gradients reach every head parameter through all 5 stacks and the loss goes down"""
    import copy
    g = golden("train_loss.npz")
    net = make_net(copy.copy(opt), "fp32")
    net.train(True)
    heads = [p for m in (net.df, net.part_predictor, net.pca_predictor, net.center_predictor) for p in m.parameters()]
    for p in heads:
        p.requires_grad_(True)
    keys = ("images", "points", "df_h", "df_o", "parts_gt", "pca_gt", "body_center", "obj_center", "crop_center")
    batch = {k: torch.from_numpy(g[k]).cuda() for k in keys}
    optim = torch.optim.Adam(heads, lr=1e-3)
    losses = []
    for _ in range(4):
        optim.zero_grad()
        error, _ = net.forward(**batch)
        error.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in heads)
        optim.step()
        losses.append(float(error))
    assert abs(losses[0] - float(g["error"])) < 1e-4 * float(g["error"])
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("mode", ["fp32", "fp16x3"])
def test_full_training_backward_matches_reference(opt, mode):
    """(mode "fp16x3", round 5: the same bound with every convolution, data gradient and weight gradient of the encoder on the
    fp16 matrix cores with hi / lo split operands and the heads on their fp16 x 3 path -- the fp32-grade training mode)
    CHORE.forward + backward with EVERY parameter trainable (encoder included) against the gradients the reference's
    autograd produced on the same batch (tests/golden/train_grads.npz): loss value, and per parameter the sum, abs-sum
    and L2 norm of the gradient, the complete gradient of every small tensor (GroupNorm affines, biases) and crops of
    three convolution kernels.  fp32 mode.  Tolerance 3e-3 of the tensor's L2 norm: the loss sums 5 x 1024 points, a
    handful of which sit on a ReLU kink of the heads, where the gradient is summation-order dependent in any fp32
    implementation (gradient parity note); everything upstream inherits that."""
    import copy
    g, gg = golden("train_loss.npz"), golden("train_grads.npz")
    net = make_net(copy.copy(opt), mode)
    net.train(True)
    for p in net.parameters():
        p.requires_grad_(True)
    keys = ("images", "points", "df_h", "df_o", "parts_gt", "pca_gt", "body_center", "obj_center", "crop_center")
    error, losses_all = net.forward(**{k: torch.from_numpy(g[k]).cuda() for k in keys})
    assert abs(float(error.detach()) - float(gg["error"])) < 1e-4 * float(gg["error"])
    np.testing.assert_allclose(losses_all.numpy(), g["losses_all"], rtol=1e-4)
    error.backward()
    params = dict(net.named_parameters())
    n_grad = n_none = 0
    worst = (0.0, "")
    rel_l2 = []
    for name in [str(n) for n in gg["names"]]:
        ref = gg["s_" + name]
        p = params[name]
        if np.isnan(ref).any():
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name      # unused bn4 (reference quirk)
            n_none += 1
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        a = p.grad.detach().cpu().numpy().astype(np.float64)
        got = np.array([a.sum(), np.abs(a).sum(), np.sqrt((a ** 2).sum())])
        l2 = ref[2]
        assert abs(got[2] - ref[2]) < 3e-3 * l2 and abs(got[1] - ref[1]) < 3e-3 * ref[1], (name, got, ref)
        assert abs(got[0] - ref[0]) < 3e-3 * max(ref[1], 1e-30), (name, got, ref)
        if "g_" + name in gg.files:
            err = np.sqrt(((a - gg["g_" + name]) ** 2).sum())
            assert err < 3e-3 * l2, (name, err, l2)
            worst = max(worst, (err / l2, name))
            rel_l2.append(err / l2)
        if "c_" + name in gg.files:
            c = a.reshape(a.shape[0], -1)[:16, :24]
            assert np.abs(c - gg["c_" + name]).max() < 3e-3 * np.abs(gg["c_" + name]).max(), name
        n_grad += 1
    assert n_grad == 475 and n_none == 82, (n_grad, n_none)
    print("mode %s: small-tensor relative L2 error of the gradients against the reference: median %.2e worst %.2e (%s)"
          % (mode, float(np.median(rel_l2)), worst[0], worst[1]))


@pytest.mark.parametrize("mode", ["fp32", "fp16x3", "bf16"])
def test_four_training_steps_follow_the_reference(opt, mode):
    """FOUR steps of the reference's Trainer.train_step sequence (trainer/trainer.py:76-85; Adam, lr 1e-4) on two alternating batches,
    against the reference's own CPU run (tests/golden/train_steps.npz, make_golden.gen_train_steps): the loss of every step -- steps
    2-4 are evaluated at parameters the earlier steps moved -- and how far every parameter tensor travelled.  Bounds: fp32 and
    fp16x3 (the fp32-grade training mode of round 5) losses 2e-4 relative, displacement norms 2 % (Adam's first steps move every
    entry by ~lr whatever its gradient's size, so an entry whose gradient is round-off noise goes either way: the NORM of a
    tensor's displacement is stable, its entries are not); bf16 losses 2e-2, norms 10 %."""
    import copy
    from make_train_batch import train_batch
    g = golden("train_steps.npz")
    net = make_net(copy.copy(opt), mode)
    net.train(True)
    for p in net.parameters():
        p.requires_grad_(True)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    batches = [{k: torch.from_numpy(v).cuda() for k, v in train_batch(seed=int(sd)).items()} for sd in g["seeds"]]
    optim = torch.optim.Adam(net.parameters(), lr=float(g["lr"]))
    errors = []
    for it in range(4):
        optim.zero_grad()
        error, _ = net.forward(**batches[it % 2])
        error.backward()
        optim.step()
        errors.append(float(error.detach()))
    ltol, ntol = (5e-3, 0.10) if mode == "bf16" else (2e-4, 0.02)      # measured: bf16 1.5e-3 / 4.4e-2, fp16x3 8.7e-5 / 3.4e-3, fp32 6.2e-5 / 3.4e-3
    rel = [abs(a - b) / b for a, b in zip(errors, g["errors"])]
    print("mode %s: losses %s | relative deviation from the reference's %s" % (mode, ["%.3f" % e for e in errors], ["%.1e" % r for r in rel]))
    assert max(rel) < ltol, (errors, list(g["errors"]))
    assert errors[-1] < 0.5 * errors[0]
    worst = (0.0, "")
    for n, p in net.named_parameters():
        ref = g["d_" + n]
        d = float((p.detach() - before[n]).double().norm())
        if ref[0] == 0.0:
            assert d == 0.0, n                      # the never-used bn4 affines stay where they are
            continue
        worst = max(worst, (abs(d - ref[0]) / ref[0], n))
    print("largest deviation of a tensor's displacement norm: %.2e (%s)" % worst)
    assert worst[0] < ntol, worst


def test_full_training_backward_bf16_mode_within_stated_bound(opt):
    """the same backward in the mode bench.py --mode train runs (bf16 activations and MFMA operands, fp32 heads and
    accumulation) against the reference's fp32 autograd gradients (tests/golden/train_grads.npz).  Stated bound: loss
    within 2e-2 relative; per parameter tensor the L2 norm and abs-sum of the gradient within 15 %, the complete small
    tensors (GroupNorm affines, biases) within 25 % of the tensor's L2 norm in L2 error, and the MEDIAN over all
    tensors of that relative error below 8 % -- bf16 carries 8 mantissa bits through ~100 layers forward and back, so
    this is a 1e-2 .. 1e-1 mode for gradients; it is what training in bf16 means, and it is measured here."""
    import copy
    g, gg = golden("train_loss.npz"), golden("train_grads.npz")
    net = make_net(copy.copy(opt), "bf16")
    net.train(True)
    for p in net.parameters():
        p.requires_grad_(True)
    keys = ("images", "points", "df_h", "df_o", "parts_gt", "pca_gt", "body_center", "obj_center", "crop_center")
    error, _ = net.forward(**{k: torch.from_numpy(g[k]).cuda() for k in keys})
    assert abs(float(error.detach()) - float(gg["error"])) < 2e-2 * float(gg["error"])
    error.backward()
    params = dict(net.named_parameters())
    rel, n_grad = [], 0
    for name in [str(n) for n in gg["names"]]:
        ref = gg["s_" + name]
        p = params[name]
        if np.isnan(ref).any():
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        a = p.grad.detach().float().cpu().numpy().astype(np.float64)
        got = np.array([a.sum(), np.abs(a).sum(), np.sqrt((a ** 2).sum())])
        assert abs(got[2] - ref[2]) < 0.15 * ref[2] and abs(got[1] - ref[1]) < 0.15 * ref[1], (name, got, ref)
        if "g_" + name in gg.files:
            err = np.sqrt(((a - gg["g_" + name]) ** 2).sum()) / ref[2]
            assert err < 0.25, (name, err)
            rel.append(err)
        n_grad += 1
    assert n_grad == 475
    print("bf16 mode: relative L2 error of the small gradient tensors: median %.3f max %.3f" % (np.median(rel), max(rel)))
    assert np.median(rel) < 0.08


def test_fused_loss_kernel_equals_tensor_op_loss(opt):
    """chore_train_loss (one kernel per stack: six terms + four gradient tensors, exact reductions) against the same loss
    written with torch ops (CHORE_TORCH_LOSS=1, the form checked against the reference by the tests above): the six terms,
    the error and its gradients with respect to all four predictions of both stacks"""
    import os
    from chore_amd.model import CHORE
    torch.manual_seed(3)
    net = CHORE(opt).cuda()
    B, N = 3, 1111
    tg = dict(df_h=torch.rand(B, N).cuda() * 0.2, df_o=torch.rand(B, N).cuda() * 0.2, parts_gt=torch.randint(0, 14, (B, N)).cuda(),
              pca_gt=torch.randn(B, 3, 3, N).cuda(), body_center=torch.randn(B, 3).cuda() * 0.3, obj_center=torch.randn(B, 3, N).cuda() * 0.3)
    res = {}
    for mode in ("fused", "torch"):
        torch.manual_seed(4)
        preds = []
        for _ in range(2):
            df = (torch.rand(B, 2, N) * 0.7).cuda()
            df[:, :, ::17] = 5.0                                   # OUT_DIST entries: clamped, no gradient
            preds.append([t.requires_grad_(True) for t in (df, torch.randn(B, 3, 3, N).cuda(), torch.randn(B, 14, N).cuda() * 2,
                                                           torch.randn(B, 6, N).cuda() * 0.3)])
        net.intermediate_preds_list = [tuple(p) for p in preds]
        if mode == "torch":
            os.environ["CHORE_TORCH_LOSS"] = "1"
        try:
            err, losses = net.get_errors(max_dist=0.5, **tg)
        finally:
            os.environ.pop("CHORE_TORCH_LOSS", None)
        (err * 1.7).backward()
        res[mode] = (err.detach(), losses.detach().cpu() if losses.is_cuda else losses, [t.grad for p in preds for t in p])
    a, b = res["fused"], res["torch"]
    assert abs(float(a[0]) - float(b[0])) <= 2e-6 * abs(float(b[0]))
    assert torch.allclose(a[1].float(), b[1].float(), rtol=2e-6, atol=0)
    for ga, gb in zip(a[2], b[2]):
        assert ga.shape == gb.shape
        assert float((ga - gb).abs().max()) <= 2e-6 * float(gb.abs().max())


def test_fp16_mode_back_to_back_encodes_have_no_slow_launches():
    """regression: with two workgroups of conv_pc_kernel's small fp16 tilings on one CU, two high-priority consumer waves per
    SIMD polling for operands starved their producers -- single launches took 25 s (50 us normally), whole encodes seconds,
    first seen as a 1 s-per-launch line in a profile.  conv_pc launches now always request more than half a CU's LDS (one
    workgroup per CU) and no wave keeps its priority while it polls.  300 encodes queued back to back, each between two
    events, in a child process with a timeout: none beyond 3x the median."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, "scripts", "fp16_outlier_probe.py"), "fp16", "300"], capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("fp16")][-1]
    assert "beyond 3x median: 0" in line, line
    assert float(line.split("median")[1].split("ms")[0]) < 8.0, line
