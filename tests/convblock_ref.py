"""The float64 reference of one ConvBlock as a training operator (csrc/convblock.hip), plain torch on the CPU, stage by stage
(tests/test_gpu_convblock_kernels.py, tests/test_convblock_coverage_table.py).

  forward    o1 = conv1(relu(gn1(x))), o2 = conv2(relu(gn2(o1))), o3 = conv3(relu(gn3(o2))), y = cat(o1, o2, o3) + res,
             res = x, or convd(relu(gn4(x))) (1x1) when Cin != Cout.  Every stage is conv_ref.forward on whatever tensor it is
             handed: the GPU module hands each stage what the device STORED, so every compared quantity is one layer deep.
  backward   three chained single-layer autograd steps plus the downsample branch:
               d(o2) = grad_o2 <conv3(relu(gn3(o2))), dy3> + dy2,   d(o1) = grad_o1 <conv2(relu(gn2(o1))), d(o2)> + dy1,
               dx = grad_x <conv1(relu(gn1(x))), d(o1)> + skip,     skip = dy, or grad_x <convd(relu(gn4(x))), dy>
             with the parameter gradients of the same steps.  `rnd` rounds what the operator stores or feeds to a matrix core in
             a 16-bit mode -- the weights, the normalised activations, each data-gradient output, d(o2), d(o1), dx4, dx -- and
             nothing else: with rnd = None it is the float64 reference, with bf16 rounding conv_ref.storage_model's extension to
             the backward chain, whose distance from the reference is the error the number format alone causes.
  nudge      stored values whose float64 pre-activation under a GroupNorm lies within KINK of the ReLU's kink are moved by the
             fewest representable steps of the storage type that give |pre| >= 2 KINK with the same sign, statistics recomputed,
             until none is left: after that no ReLU branch depends on the device's rounding, and nothing needs masking.
             o1 / o2 are nudged in `saved` AFTER the forward took their statistics, and the cells stay: bn2 / bn3 then normalise
             the nudged tensor with the statistics of the stored one.  The reference does the same (`stats`): the GroupNorm
             backward is written out with the statistics as an argument, and equals autograd's when they are the tensor's own.

Tensors are NHWC (numpy, or torch of the storage type), weights in the reference layout (O, C, kh, kw), params a dict with
w1 w2 w3 [wd] g1 b1 g2 b2 g3 b3 [g4 b4] as float32 numpy."""
import numpy as np
import torch
import torch.nn.functional as F

import conv_ref

EPS = 1e-5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _nchw(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).double().permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def bf16_round(t):
    return t.to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------ forward
def stage(x_stored, w, gamma, beta):
    """conv(relu(gn(x))) of a stored NHWC tensor -> float64 numpy NHWC"""
    return conv_ref.forward(x_stored, w, None, gamma, beta)


def forward(x_stored, p, mode="fp32"):
    """the whole block in float64, every intermediate rounded to the storage type of `mode` as the operator stores it
    -> dict o1, o2 (torch, storage type), y (float64 numpy, unrounded last step)"""
    st = conv_ref.STORAGE[mode]
    o1 = stage(x_stored, p["w1"], p["g1"], p["b1"])
    o1s = torch.from_numpy(o1).to(st)
    o2 = stage(o1s, p["w2"], p["g2"], p["b2"])
    o2s = torch.from_numpy(o2).to(st)
    o3 = stage(o2s, p["w3"], p["g3"], p["b3"])
    res = stage(x_stored, p["wd"], p["g4"], p["b4"]) if "wd" in p else x_stored.double().numpy()
    return dict(o1=o1s, o2=o2s, y=np.concatenate([o1s.double().numpy(), o2s.double().numpy(), o3], -1) + res)


# ------------------------------------------------------------------------------------------------ GroupNorm, statistics given
def group_stats(t_stored):
    """(mean, biased variance) per (image, group) of a stored NHWC tensor, float64 torch tensors of shape (B, 32, 1, 1)"""
    x = _nchw(t_stored)
    B, C = x.shape[:2]
    g = x.reshape(B, 32, -1)
    return g.mean(2).reshape(B, 32, 1, 1), g.var(2, unbiased=False).reshape(B, 32, 1, 1)


def _normalise(x, gamma, beta, stats):
    """x NCHW float64 -> (xhat, pre-activation, rstd per channel), all NCHW-broadcastable; the statistics are the given ones: the
    operator normalises with the statistics CELLS it is handed, whatever tensor they were taken from"""
    B, C = x.shape[:2]
    gs = C // 32
    mean, var = stats
    mean = mean.repeat_interleave(gs, 1)
    rstd = (1.0 / torch.sqrt(var + EPS)).repeat_interleave(gs, 1)
    xhat = (x - mean) * rstd
    return xhat, xhat * _t(gamma).reshape(1, C, 1, 1) + _t(beta).reshape(1, C, 1, 1), rstd


def _group_mean(t):
    B, C, H, W = t.shape
    return t.reshape(B, 32, -1).mean(2).reshape(B, 32, 1, 1).repeat_interleave(C // 32, 1)


# ------------------------------------------------------------------------------------------------ backward
def _layer_bwd(x_stored, gamma, beta, w, dout, rnd, stats=None):
    """one GroupNorm -> ReLU -> conv layer: dout (NCHW float64) -> (gradient to x through the layer, unrounded; dW; dgamma; dbeta).
    stats: the statistics the GroupNorm uses (None: those of x_stored itself, and then this is autograd's result)"""
    r = rnd or (lambda t: t)
    x = _nchw(x_stored)
    xhat, pre, rstd = _normalise(x, gamma, beta, stats or group_stats(x_stored))
    live = (pre > 0).double()
    a = pre * live
    w64 = _t(w)
    k = w64.shape[-1]
    da = r(F.conv_transpose2d(dout, r(w64), padding=k // 2))            # the stored data gradient
    wz = torch.zeros_like(w64).requires_grad_(True)                     # (dW does not depend on w)
    F.conv2d(r(a), wz, padding=k // 2).backward(dout)
    g = da * live
    gy = g * _t(gamma).reshape(1, -1, 1, 1)
    dx = rstd * (gy - _group_mean(gy) - xhat * _group_mean(gy * xhat))
    return dx, wz.grad.numpy(), (g * xhat).sum((0, 2, 3)).numpy(), g.sum((0, 2, 3)).numpy()


def backward(x_stored, o1_stored, o2_stored, dy_stored, p, rnd=None, stats=None):
    """-> dict dx (NHWC), dw1 dw2 dw3 [dwd], dg1 db1 dg2 db2 dg3 db3 [dg4 db4], float64 numpy.
    stats: {"o1": ..., "o2": ...} statistics (group_stats) bn2 / bn3 normalise with, where they are not those of the tensors handed in"""
    r = rnd or (lambda t: t)
    stats = stats or {}
    dy = _nchw(dy_stored)
    cout = dy.shape[1]
    c1, c2 = cout // 2, cout // 4
    dy1, dy2, dy3 = dy[:, :c1], dy[:, c1:c1 + c2], dy[:, c1 + c2:]
    out = {}
    g, out["dw3"], out["dg3"], out["db3"] = _layer_bwd(o2_stored, p["g3"], p["b3"], p["w3"], dy3.contiguous(), rnd, stats.get("o2"))
    do2 = r(g + dy2)
    g, out["dw2"], out["dg2"], out["db2"] = _layer_bwd(o1_stored, p["g2"], p["b2"], p["w2"], do2, rnd, stats.get("o1"))
    do1 = r(g + dy1)
    if "wd" in p:
        g, out["dwd"], out["dg4"], out["db4"] = _layer_bwd(x_stored, p["g4"], p["b4"], p["wd"], dy, rnd)
        skip = r(g)
    else:
        skip = dy
    g, out["dw1"], out["dg1"], out["db1"] = _layer_bwd(x_stored, p["g1"], p["b1"], p["w1"], do1, rnd)
    out["dx"] = _nhwc(r(g + skip))
    return out


def backward_autograd(x_stored, o1_stored, o2_stored, dy_stored, p):
    """the same gradients from torch.autograd on the three chained layers and the downsample branch (statistics of the tensors
    handed in): what `backward` must equal when no statistics are given"""
    def layer(t_stored, g, b, w, dout):
        x = _nchw(t_stored).requires_grad_(True)
        gg, bb, ww = _t(g).requires_grad_(True), _t(b).requires_grad_(True), _t(w).requires_grad_(True)
        F.conv2d(F.relu(F.group_norm(x, 32, gg, bb, eps=EPS)), ww, padding=ww.shape[-1] // 2).backward(dout)
        return x.grad, ww.grad.numpy(), gg.grad.numpy(), bb.grad.numpy()
    dy = _nchw(dy_stored)
    cout = dy.shape[1]
    c1, c2 = cout // 2, cout // 4
    out = {}
    g, out["dw3"], out["dg3"], out["db3"] = layer(o2_stored, p["g3"], p["b3"], p["w3"], dy[:, c1 + c2:].contiguous())
    do2 = g + dy[:, c1:c1 + c2]
    g, out["dw2"], out["dg2"], out["db2"] = layer(o1_stored, p["g2"], p["b2"], p["w2"], do2)
    do1 = g + dy[:, :c1]
    skip = dy
    if "wd" in p:
        skip, out["dwd"], out["dg4"], out["db4"] = layer(x_stored, p["g4"], p["b4"], p["wd"], dy)
    g, out["dw1"], out["dg1"], out["db1"] = layer(x_stored, p["g1"], p["b1"], p["w1"], do1)
    out["dx"] = _nhwc(g + skip)
    return out


# ------------------------------------------------------------------------------------------------ ReLU kinks
def pre_activation(t_stored, gamma, beta, stats=None):
    """the GroupNorm's output in float64 (statistics: the given ones, else those of the stored tensor), NHWC numpy"""
    return _nhwc(_normalise(_nchw(t_stored), gamma, beta, stats or group_stats(t_stored))[1])


def _toward(v, target, up):
    """the value of v's type nearest to `target` (float64) that is not short of it in the direction `up`"""
    c = torch.from_numpy(target).to(v.dtype)
    short = torch.from_numpy(np.where(up, c.double().numpy() < target, c.double().numpy() > target))
    if short.any():
        # one step of the storage type further: through the float32 bit pattern (bf16: its upper 16 bits)
        f = c.float().numpy().copy()
        bits = f.view(np.int32)
        step = np.int32(1 << 16) if v.dtype == torch.bfloat16 else np.int32(1)
        away = (f > 0) == up                      # the step raises the magnitude
        zero = f == 0
        nb = np.where(away, bits + step, bits - step)
        tiny = np.float32(2.0 ** -126).view(np.int32)
        nb = np.where(zero, np.where(up, tiny, tiny | np.int32(-2 ** 31)), nb)
        c = torch.where(short, torch.from_numpy(nb.view(np.float32)).to(v.dtype), c)
    return c


def nudge(t_stored, norms, kink, stats=None, max_rounds=20):
    """t_stored: NHWC torch tensor of the storage type; norms: [(gamma, beta)] of the GroupNorms that read it; stats: the statistics
    those GroupNorms will use (held while the tensor moves), None: the tensor's own, recomputed every round
    -> (nudged tensor, boolean NHWC mask of the moved elements, rounds)"""
    t = t_stored.clone()
    moved = np.zeros(tuple(t.shape), bool)
    for rounds in range(max_rounds + 1):
        dirty = False
        for gamma, beta in norms:
            st = stats or group_stats(t)
            pre = pre_activation(t, gamma, beta, st)
            m = np.abs(pre) < kink
            if not m.any():
                continue
            assert rounds < max_rounds, "kinks left after %d rounds" % rounds
            dirty = True
            x = t.double().numpy()
            rstd = _nhwc((1.0 / torch.sqrt(st[1] + EPS)).repeat_interleave(x.shape[-1] // 32, 1).expand(x.shape[0], -1, x.shape[1], x.shape[2]))
            slope = rstd * gamma.astype(np.float64)        # d pre / d x (statistics held)
            up = (pre >= 0) == (slope > 0)
            want = np.where(pre >= 0, 2 * kink, -2 * kink)
            # (a hair beyond the target: the statistics move with the tensor)
            target = np.where(m, x + (want - pre) / slope * (1 + 1e-6), x)
            new = _toward(t, target, up)
            t = torch.where(torch.from_numpy(m), new, t)
            moved |= m
        if not dirty:
            return t, moved, rounds
    raise AssertionError("unreachable")


def kinks(t_stored, norms, kink, stats=None):
    """number of elements within `kink` of a ReLU kink under any of the norms"""
    return int(sum((np.abs(pre_activation(t_stored, g, b, stats)) < kink).sum() for g, b in norms))


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(case):
    """x, the block's parameters and dy (standard normal times the case's dy_scale) as float32 numpy, drawn as
    test_gpu_conv_kernels.make_inputs draws its "gn" kind, seeded by the case id -> (x, params, dy)"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    B, H, W, cin, cout = (case[k] for k in ("B", "H", "W", "cin", "cout"))
    c1, c2 = cout // 2, cout // 4
    x = (rng.standard_normal((B, H, W, cin), dtype=np.float32) * 1.5 + 0.3).astype(np.float32)
    p = {}
    layers = [("1", cin, c1, 3), ("2", c1, c2, 3), ("3", c2, c2, 3)] + ([("d", cin, cout, 1)] if cin != cout else [])
    for tag, ci, co, k in layers:
        n = "4" if tag == "d" else tag
        p["w" + tag] = (rng.standard_normal((co, ci, k, k), dtype=np.float32) / np.sqrt(ci * k * k)).astype(np.float32)
        p["g" + n] = (rng.random(ci, dtype=np.float32) + 0.5).astype(np.float32)
        p["b" + n] = (rng.standard_normal(ci, dtype=np.float32) * 0.2).astype(np.float32)
    dy = rng.standard_normal((B, H, W, cout), dtype=np.float32) * np.float32(case["dy_scale"])
    return x, p, dy


def x_norms(p):
    return [(p["g1"], p["b1"])] + ([(p["g4"], p["b4"])] if "wd" in p else [])


def variant_dy(dy, cout, variant):
    """the dy of a variant of convblock_cases.VARIANTS: (slices kept, scale of the third slice)"""
    keep, s3 = variant
    c1, c2 = cout // 2, cout // 4
    out = np.zeros_like(dy)
    for k, (lo, hi) in enumerate(((0, c1), (c1, c1 + c2), (c1 + c2, cout))):
        if k in keep:
            out[..., lo:hi] = dy[..., lo:hi] * np.float32(s3 if k == 2 else 1.0)
    return out
