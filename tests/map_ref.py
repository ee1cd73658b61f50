"""Float64 references of the encoder's map operators (tests/test_gpu_map_kernels.py, tests/test_map_coverage_table.py): plain
torch / numpy on the CPU.  Tensors are NHWC like the device's, (B, H, W, C) or (B, HW, C), float64 numpy unless stated."""
import numpy as np
import torch
import torch.nn.functional as F

GROUPS = 32
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ULP = {"f32": 0.0, "bf16": 2.0 ** -7, "f16": 2.0 ** -10}      # one unit in the last place, relative


def stored(a, dtype):
    """a float32 array rounded to the storage type -> torch tensor of that type (what the device reads)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH_DTYPE[dtype])


def representable(a, dtype):
    """every entry of the float64 array survives a round trip through the storage type"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return bool((t.to(TORCH_DTYPE[dtype]).double() == t).all())


# ---- the statistics cells of csrc/enc_common.h: [2 tables][B][32 groups] GroupStat {sum, sq}, a cell {u64 lo, i64 hi};
# value = (table 1's hi * 2^32 + table 0's lo) * 2^-40, the other two limbs unused
def stats_cells(raw):
    """bytes of an accumulator array (uint8 numpy or a tensor) -> the value of every cell, flat (B * 32 * 2), float64; exact
    wherever the value has at most 53 significant bits"""
    if isinstance(raw, torch.Tensor):
        raw = raw.cpu().numpy()
    w = np.ascontiguousarray(raw).view(np.uint64).reshape(2, -1, 2)
    lo, hi = w[0, :, 0], w[1, :, 1].view(np.int64)
    return np.array([(int(h) * 2 ** 32 + int(l)) / 2 ** 40 for l, h in zip(lo, hi)], dtype=np.float64)


def stats_decode(raw, B):
    """-> sum, sq (B, 32)"""
    v = stats_cells(raw).reshape(B, GROUPS, 2)
    return v[..., 0], v[..., 1]


def stats_encode(ssum, ssq):
    """sum, sq (B, 32) float64 -> the bytes of the accumulator array (uint8 numpy), each value rounded to the unit 2^-40"""
    B = ssum.shape[0]
    v = np.stack([ssum, ssq], -1).reshape(-1)
    w = np.zeros((2, v.size, 2), np.uint64)
    for i, x in enumerate(v):
        total = int(round(float(x) * 2.0 ** 40))        # (a power of two: the product is exact)
        hi, lo = divmod(total, 2 ** 32)
        w[0, i, 0] = lo
        w[1, i, 1] = np.int64(hi).view(np.uint64)
    assert w.nbytes == 2 * B * GROUPS * 32
    return w.reshape(-1).view(np.uint8)


def group_stats(x):
    """x (B, ..., C) float64, the values as stored -> sum, sq (B, 32), and sum |v| per group (for the error bounds)"""
    B, C = x.shape[0], x.shape[-1]
    g = x.reshape(B, -1, GROUPS, C // GROUPS)
    return g.sum((1, 3)), (g * g).sum((1, 3)), np.abs(g).sum((1, 3))


def gn_relu(x, gamma, beta):
    """relu(F.group_norm(x, 32, gamma, beta, 1e-5)) of x (B, HW, C)"""
    t = torch.from_numpy(x).permute(0, 2, 1)
    y = F.relu(F.group_norm(t, GROUPS, torch.from_numpy(gamma), torch.from_numpy(beta), eps=1e-5))
    return y.permute(0, 2, 1).contiguous().numpy()


def avgpool2(x):
    """F.avg_pool2d(x, 2, 2) of x (B, H, W, C)"""
    return F.avg_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 2, stride=2).permute(0, 2, 3, 1).contiguous().numpy()


def avgpool2_bwd(dy):
    """its transpose: every dy / 4 into its four inputs"""
    return np.repeat(np.repeat(dy, 2, axis=1), 2, axis=2) * 0.25


# ---- bicubic x2, align_corners=True, A = -0.75, border-clamped taps, written out as a matrix per axis
def cubic_coeffs(t):
    A = -0.75
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    return (((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A, ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0,
            ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0, ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A)


def up2_matrix(n):
    """(2 n, n): row o holds the weights of output coordinate o on the n source coordinates; source coordinate o (n - 1) / (2 n - 1)"""
    M = np.zeros((2 * n, n))
    for o in range(2 * n):
        r = o * (n - 1) / (2 * n - 1)          # the numerator is an integer: exact at o = 0 and at o = 2 n - 1
        i = int(np.floor(r))
        for k, c in enumerate(cubic_coeffs(r - i)):
            M[o, min(max(i - 1 + k, 0), n - 1)] += c
    return M


def upadd(a, low):
    """a + U low: a (B, 2H, 2W, C), low (B, H, W, C); x first, then y"""
    My, Mx = up2_matrix(low.shape[1]), up2_matrix(low.shape[2])
    rows = np.einsum("pw,bhwc->bhpc", Mx, low)
    return a + np.einsum("oh,bhpc->bopc", My, rows)


def up2_bwd(dy):
    """U^T dy: dy (B, 2H, 2W, C) -> (B, H, W, C)"""
    My, Mx = up2_matrix(dy.shape[1] // 2), up2_matrix(dy.shape[2] // 2)
    return np.einsum("oh,bopc->bhpc", My, np.einsum("pw,bopc->bowc", Mx, dy))


def stem(img, w, bias):
    """F.conv2d(stride 2, padding 3) of img (B, Cin, H, W) -> y (B, H/2, W/2, 64), and the same convolution of |w| and |x| (no bias)"""
    ti, tw = torch.from_numpy(np.asarray(img, np.float64)), torch.from_numpy(np.asarray(w, np.float64))
    y = F.conv2d(ti, tw, torch.from_numpy(np.asarray(bias, np.float64)), stride=2, padding=3)
    ya = F.conv2d(ti.abs(), tw.abs(), None, stride=2, padding=3)
    return y.permute(0, 2, 3, 1).contiguous().numpy(), ya.permute(0, 2, 3, 1).contiguous().numpy()


def absmax_bits(x):
    """the float bits of max |x| of a float32 array"""
    return int(np.abs(np.asarray(x, np.float32)).max().view(np.uint32)) if x.size else 0
