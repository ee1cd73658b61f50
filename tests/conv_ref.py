"""The float64 reference of one encoder convolution layer, plain torch on the CPU (tests/test_gpu_conv_kernels.py,
tests/test_gpu_wgrad_kernels.py).

  forward          y = conv2d(a, w, zero padding) + bias,  a = relu(group_norm(x, 32, gamma, beta, eps=1e-5)) when GroupNorm is fused
  data gradient    dx = conv_transpose2d(dy, w)   (= the convolution of dy with the transposed, spatially flipped weights)
  weight gradient  dW, dbias of that forward for an upstream gradient dy, by autograd

Tensors are NHWC numpy arrays (what the kernels read), weights in the reference layout (O, C, kh, kw).  Everything is computed
in float64 from the bits the device is handed: a 16-bit mode's reference sees the input rounded to the storage type first
(`as_stored`), exactly as test_gpu_train_ops.py::test_conv_gn_layer does for bf16.

`storage_model` is the error model of a 16-bit storage mode: the same layer with the normalised activation and the output
rounded to the storage type and nothing else (exact weights, exact accumulation).  Its distance from the float64 result is the
error the number format alone causes; the fp16 bound of the matrix is derived from it (the project states no per-layer fp16
bound)."""
import numpy as np
import torch
import torch.nn.functional as F

STORAGE = {"fp32": torch.float32, "x3": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def as_stored(x, mode):
    """x (numpy, float32) rounded to the storage type of `mode`, as a torch tensor of that type"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(STORAGE[mode])


def _nchw64(t):
    return t.double().permute(0, 3, 1, 2).contiguous()


def normalised(x_stored, gamma, beta):
    """relu(group_norm(x)) in float64, NCHW; x_stored: NHWC torch tensor of the storage type"""
    return F.relu(F.group_norm(_nchw64(x_stored), 32, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), eps=1e-5))


def _conv(a, w, bias):
    w = torch.from_numpy(w).double()
    b = None if bias is None else torch.from_numpy(bias).double()
    return F.conv2d(a, w, b, padding=w.shape[-1] // 2)


def forward(x_stored, w, bias=None, gamma=None, beta=None):
    """-> y (B, H, W, Cout) float64 numpy"""
    a = normalised(x_stored, gamma, beta) if gamma is not None else _nchw64(x_stored)
    return _conv(a, w, bias).permute(0, 2, 3, 1).contiguous().numpy()


def data_gradient(dy_stored, w):
    """dy (B, H, W, Cout) of the storage type, w (Cout, Cin, kh, kw) -> dx (B, H, W, Cin) float64 numpy"""
    w = torch.from_numpy(w).double()
    dx = F.conv_transpose2d(_nchw64(dy_stored), w, padding=w.shape[-1] // 2)
    return dx.permute(0, 2, 3, 1).contiguous().numpy()


def weight_gradient(x_stored, dy_stored, k, gamma=None, beta=None):
    """x (B, H, W, Cin), dy (B, H, W, Cout) of the storage type -> dW (Cout, Cin, k, k), dbias (Cout), float64 numpy: autograd of
    conv2d(a, w) + bias, a = relu(group_norm(x)) with gamma / beta, else x"""
    a = normalised(x_stored, gamma, beta) if gamma is not None else _nchw64(x_stored)
    w = torch.zeros(dy_stored.shape[-1], a.shape[1], k, k, dtype=torch.float64, requires_grad=True)     # (dW does not depend on w)
    b = torch.zeros(dy_stored.shape[-1], dtype=torch.float64, requires_grad=True)
    F.conv2d(a, w, b, padding=k // 2).backward(_nchw64(dy_stored))
    return w.grad.numpy(), b.grad.numpy()


def storage_model(x_stored, w, bias, gamma, beta, mode):
    """the forward layer with the normalised activation and the output rounded to the storage type of `mode` -> float64 numpy"""
    t = STORAGE[mode]
    a = normalised(x_stored, gamma, beta) if gamma is not None else _nchw64(x_stored)
    a = a.to(t).double()
    y = _conv(a, w, bias).to(t).double()
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def group_sums(y_stored, groups=32):
    """per image and GroupNorm group of a stored output (B, H, W, C): (sum, sum of squares) in float64 -> (B * groups, 2),
    the order of the library's statistics cells (stat_values)"""
    y = np.asarray(y_stored, dtype=np.float64)
    B, H, W, C = y.shape
    g = y.reshape(B, H * W, groups, C // groups)
    return np.stack([g.sum((1, 3)), (g * g).sum((1, 3))], -1).reshape(B * groups, 2)


def stat_values(cells):
    """the library's statistics cells, [2 tables][B][32] GroupStat (sum, sq) x (lo, hi) limbs as int64 -> (B * 32, 2) totals as
    float64 (enc_common.h stat_read)"""
    c = cells.reshape(2, -1, 2, 2)               # table, (image, group), sum / sq, limb
    lo = c[0, :, :, 0].astype(np.uint64)
    top = c[1, :, :, 1].astype(np.float64) + (lo >> np.uint64(32)).astype(np.float64)
    return (top * 2.0 ** 32 + (lo & np.uint64(0xffffffff)).astype(np.float64)) * 2.0 ** -40


def rel_max(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
