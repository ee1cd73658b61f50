"""GPU: the backward operators of the training step that are no convolution layer -- chore_gn_relu_bwd, chore_gemm_tn_f32,
chore_stem_bwd_weight (csrc/train_bwd.hip) and chore_heads_wgrad (csrc/heads_wgrad.hip) -- called directly through the C API and
compared with plain torch in float64 on the CPU.  (The weight gradients of the convolution layers: tests/test_gpu_wgrad_kernels.py.)

Bounds, as everywhere for a single operator (test_gpu_train_ops.py): fp32 within 2e-5 of the reference's largest entry; bf16
(16-bit storage, fp32 accumulation) within 3e-2 of it and 1.5e-2 relative L2, the reference fed the bf16-rounded tensors; the
heads' parameter gradients within 5e-5 of each tensor's largest entry (test_training_backward_heads_and_feature_maps).  Inputs in
{-1, 0, 1} must come out bit for bit (a zero's sign aside): every partial sum is a small integer, in the fp16 x 3 arithmetic an
integer times a power of two.  Outputs live between sentinel margins and are pre-filled with NaN; workspaces have exactly the size
their *_bytes function states, plus a sentinel page (tests/gpu_guards.py, shared with test_gpu_fit_kernels.py).

Measured on an MI355X (worst max error / relative L2 over the cases, next to the bound on the max; the module takes 7 s):
  chore_gn_relu_bwd      fp32  dx 1.6e-06 / 9.0e-07, dgamma 5.6e-07 / 2.5e-07, dbeta 1.6e-07 / 1.2e-07 (2e-5), all at C = 32, HW = 4 or 129
                         bf16  dx 3.6e-03 / 1.7e-03, dgamma 2.6e-07 / 1.1e-07, dbeta 5.0e-08 / 1.5e-08 (3e-2, L2 1.5e-2)
                         ReLU kinks masked: 0.39 % of the entries at worst (C = 32, HW = 4: one of 256), 0.1 % typically
  chore_gemm_tn_f32      2.8e-07 / 2.1e-07 (2e-5) at P = 1000, M = 128, N = 96
  chore_stem_bwd_weight  fp32  dw 3.4e-07 / 2.7e-07, dbias 2.6e-07 / 2.5e-07 (2e-5);  bf16  dw 3.0e-07 / 2.7e-07, dbias 9.1e-08 / 7.6e-08 (3e-2)
  chore_heads_wgrad      6.7e-07 / 5.2e-07 (5e-5) in both arithmetic modes, at P = 831 in the bias of an output layer
  every exact case, guard margin and workspace page held.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_guards import Guarded, Workspace, _close, _exact

pytestmark = pytest.mark.gpu

F32_BOUND, BF16_BOUND, BF16_L2, HEADS_BOUND = 2e-5, 3e-2, 1.5e-2, 5e-5


def _env():
    from chore_amd import _lib
    dev = torch.device("cuda", 0)
    return _lib, _lib.lib, _lib.handle(0), dev, torch.cuda.current_stream(dev).cuda_stream


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ================================================================================================ chore_gn_relu_bwd
KINK = 1e-3


def _gn_case(C, HW, B, dtype):
    """inputs (as stored) and the float64 reference of relu(group_norm(x)) backward"""
    rng = _rng("gn", C, HW, B, str(dtype))
    x = torch.from_numpy(rng.standard_normal((B, HW, C), dtype=np.float32) * 1.5 + 0.3).to(dtype)
    da = torch.from_numpy(rng.standard_normal((B, HW, C), dtype=np.float32)).to(dtype)
    gamma = torch.from_numpy(rng.random(C, dtype=np.float32) + 0.5)       # in [0.5, 1.5): the pre-activation's density at 0 stays below 0.8
    beta = torch.from_numpy(rng.standard_normal(C, dtype=np.float32) * 0.2)
    x64 = x.double().permute(0, 2, 1).contiguous().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pre = F.group_norm(x64, 32, g64, b64, eps=1e-5)
    # ReLU kinks: no upstream gradient where the pre-activation is this close to 0 -- the result then does not depend on which
    # branch the device's fp32 pre-activation took there
    kink = (pre.detach().abs() < KINK).permute(0, 2, 1)
    share = kink.double().mean().item()
    assert share <= 0.01, (C, HW, B, share)
    da = torch.where(kink, torch.zeros_like(da), da)
    F.relu(pre).backward(da.double().permute(0, 2, 1))
    ref = (x64.grad.permute(0, 2, 1).contiguous().numpy(), g64.grad.numpy(), b64.grad.numpy())
    return x, da, gamma, beta, ref, share


def _gn_run(x, da, gamma, beta, zeroed):
    _lib, L, h, dev, stream = _env()
    B, HW, C = x.shape
    dt = _lib.F32 if x.dtype == torch.float32 else _lib.BF16
    xd, dad, gd, bd = x.to(dev).contiguous(), da.to(dev).contiguous(), gamma.to(dev), beta.to(dev)
    st = torch.zeros(L.chore_gn_stats_bytes(B), dtype=torch.uint8, device=dev)
    _lib.check(L.chore_gn_stats(h, dt, xd.data_ptr(), B, HW, C, st.data_ptr(), 1, stream), h, "gn_stats")
    dx, dg, db = Guarded(B * HW * C, dev, x.dtype), Guarded(C, dev), Guarded(C, dev)
    ws = Workspace(L.chore_gn_relu_bwd_workspace_bytes(B, C), dev, zero=bool(zeroed))
    _lib.check(L.chore_gn_relu_bwd(h, dt, xd.data_ptr(), st.data_ptr(), gd.data_ptr(), bd.data_ptr(), dad.data_ptr(), B, HW, C, dx.ptr,
                                   dg.ptr, db.ptr, ws.ptr, zeroed, stream), h, "gn_relu_bwd")
    torch.cuda.synchronize()
    ws.check("gn_relu_bwd")
    return dx.read("dx").reshape(B, HW, C), dg.read("dgamma"), db.read("dbeta")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [4, 100, 129, 384, 9216])      # 9216: 72 shares of 128 pixels, clamped to GN_SPLITS_MAX = 64
@pytest.mark.parametrize("C", [32, 64, 128, 256])            # 32: one channel per group, the special lane of gn_bwd_reduce_kernel
def test_gn_relu_bwd(C, HW, B, dtype):
    x, da, gamma, beta, ref, share = _gn_case(C, HW, B, dtype)
    bf = dtype == torch.bfloat16
    for zeroed in (0, 1):          # 0: the operator clears a workspace full of garbage itself; 1: the caller hands it zeros
        got = _gn_run(x, da, gamma, beta, zeroed)
        for name, g, r in zip(("dx", "dgamma", "dbeta"), got, ref):
            _close(g, r, "gn_relu_bwd.%s C %d HW %d B %d zeroed %d (kinks %.2f %%)" % (name, C, HW, B, zeroed, 100 * share),
                   BF16_BOUND if bf else F32_BOUND, BF16_L2 if bf else None)
    # no upstream gradient at all: exactly nothing comes back
    for g in _gn_run(x, torch.zeros_like(da), gamma, beta, 0):
        assert not g.any(), (C, HW, B, float(np.abs(g).max()))


def test_gn_relu_bwd_refuses_96_channels():
    _lib, L, h, dev, stream = _env()
    B, HW, C = 1, 100, 96
    x = torch.zeros(B, HW, C, device=dev)
    st = torch.zeros(L.chore_gn_stats_bytes(B), dtype=torch.uint8, device=dev)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    dx, dg, db = Guarded(B * HW * C, dev, fill=3.0), Guarded(C, dev, fill=3.0), Guarded(C, dev, fill=3.0)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    rc = L.chore_gn_relu_bwd(h, _lib.F32, x.data_ptr(), st.data_ptr(), gamma.data_ptr(), beta.data_ptr(), x.data_ptr(), B, HW, C, dx.ptr,
                             dg.ptr, db.ptr, ws.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert rc == -1 and b"unsupported C=96" in L.chore_last_error(h)
    for t in (dx, dg, db):
        assert (t.read("refused call") == 3.0).all()


# ================================================================================================ chore_gemm_tn_f32
def _last_wgrad(L, h):
    rec = (ctypes.c_int * 8)()
    assert L.chore_debug_last_wgrad(h, rec, 8) == 8
    return list(rec)


@pytest.mark.parametrize("M,N", [(32, 32), (128, 96)])
@pytest.mark.parametrize("P", [1, 31, 33, 1000])
def test_gemm_tn(P, M, N):
    """C = A^T B with row strides wider than the rows; the stride padding holds NaN and must not reach the result"""
    _lib, L, h, dev, stream = _env()
    lda, ldb = M + 8, N + 4
    for kind in ("random", "exact"):
        rng = _rng("gemm", P, M, N, kind)
        A, Bm = np.full((P, lda), np.nan, np.float32), np.full((P, ldb), np.nan, np.float32)
        if kind == "random":
            A[:, :M], Bm[:, :N] = rng.standard_normal((P, M), dtype=np.float32), rng.standard_normal((P, N), dtype=np.float32)
        else:
            A[:, :M], Bm[:, :N] = rng.integers(-1, 2, (P, M)), rng.integers(-1, 2, (P, N))
        ref = A[:, :M].astype(np.float64).T @ Bm[:, :N].astype(np.float64)
        Ad, Bd = torch.from_numpy(A).to(dev), torch.from_numpy(Bm).to(dev)
        C = Guarded(M * N, dev)
        ws = Workspace(L.chore_gemm_tn_workspace_bytes(P, M, N), dev)
        before = _last_wgrad(L, h)[7]
        _lib.check(L.chore_gemm_tn_f32(h, Ad.data_ptr(), lda, Bd.data_ptr(), ldb, P, M, N, C.ptr, ws.ptr, stream), h, "gemm_tn")
        torch.cuda.synchronize()
        ws.check("gemm_tn")
        got = C.read("C").reshape(M, N)
        what = "gemm_tn P %d M %d N %d %s" % (P, M, N, kind)
        assert np.isfinite(got).all(), what
        if kind == "random":
            _close(got, ref, what, F32_BOUND)
        else:
            _exact(got, ref, what)
        # the witness: wgrad_kernel<float, 1> on 32-channel tiles, the row ("w32", "fp32", 1, "gemm_tn") of wgrad_cases.COVERAGE
        rec = _last_wgrad(L, h)
        assert rec[:4] == [1, _lib.F32, 1, 32] and rec[6] == 0 and rec[7] == before + 1, rec
        assert 1 <= rec[4] <= max(1, rec[5]) and rec[5] == ((P + 31) // 32 + 7) // 8, rec


def test_gemm_tn_refusals():
    _lib, L, h, dev, stream = _env()
    a = torch.zeros(64 * 64, device=dev)
    C = Guarded(64 * 64, dev, fill=3.0)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    assert L.chore_gemm_tn_workspace_bytes(16, 48, 32) == 0
    for lda, ldb, M, N in ((48, 32, 48, 32), (32, 48, 32, 48), (34, 32, 32, 32), (32, 38, 32, 32)):     # M % 32, N % 32, lda % 4, ldb % 4
        rc = L.chore_gemm_tn_f32(h, a.data_ptr(), lda, a.data_ptr(), ldb, 16, M, N, C.ptr, ws.data_ptr(), stream)
        assert rc == -1, (lda, ldb, M, N, rc)
    torch.cuda.synchronize()
    assert (C.read("refused call") == 3.0).all()


# ================================================================================================ chore_stem_bwd_weight
def _stem_ref(img, dy_stored):
    """img (B,Cin,H,W) float32 numpy, dy (B,H/2,W/2,64) torch of the storage type -> dW (64,Cin,7,7), dbias (64) float64"""
    w = torch.zeros(64, img.shape[1], 7, 7, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    F.conv2d(torch.from_numpy(img).double(), w, b, stride=2, padding=3).backward(dy_stored.double().permute(0, 3, 1, 2))
    return w.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,kind", [((1, 5, 384, 384), "random"),       # 24 x 24 = 576 tiles of 8 x 8: more than the 512 shares
                                        ((1, 5, 22, 18), "exact")])         # ragged tiles, {-1, 0, 1}
def test_stem_bwd_weight(shape, kind, dtype):
    _lib, L, h, dev, stream = _env()
    B, Cin, H, W = shape
    rng = _rng("stem", shape, kind)
    if kind == "random":
        img, dy = rng.standard_normal(shape, dtype=np.float32), rng.standard_normal((B, H // 2, W // 2, 64), dtype=np.float32)
    else:
        img, dy = rng.integers(-1, 2, shape).astype(np.float32), rng.integers(-1, 2, (B, H // 2, W // 2, 64)).astype(np.float32)
    dys = torch.from_numpy(dy).to(dtype)
    ref = _stem_ref(img, dys)
    imgd, dyd = torch.from_numpy(img).to(dev), dys.to(dev).contiguous()
    dw, db = Guarded(64 * Cin * 49, dev), Guarded(64, dev)
    nws = L.chore_stem_wgrad_workspace_bytes(B, Cin, H, W)
    ntile = B * ((H // 2 + 7) // 8) * ((W // 2 + 7) // 8)
    assert nws == min(ntile, 512) * 256 * 64 * 4 and (ntile > 512) == (kind == "random")
    ws = Workspace(nws, dev)
    _lib.check(L.chore_stem_bwd_weight(h, _lib.F32 if dtype == torch.float32 else _lib.BF16, imgd.data_ptr(), B, Cin, H, W, dyd.data_ptr(),
                                       dw.ptr, db.ptr, ws.ptr, stream), h, "stem_bwd_weight")
    torch.cuda.synchronize()
    ws.check("stem_bwd_weight")
    bf = dtype == torch.bfloat16
    for name, g, r in (("dw", dw.read("dw").reshape(64, Cin, 7, 7), ref[0]), ("dbias", db.read("dbias"), ref[1])):
        what = "stem.%s %s %s" % (name, shape, kind)
        if kind == "exact":
            _exact(g, r, what)
        else:
            _close(g, r, what, BF16_BOUND if bf else F32_BOUND, BF16_L2 if bf else None)


# ================================================================================================ chore_heads_wgrad
HEAD_OUT = (2, 14, 9, 6)         # kernel head order: df, parts, pca, centers
HID, KIN, KPAD = 128, 323, 328
_HEADS = {}


def _heads_case(B, N, kind):
    """staging (X [P][328] | H [3][4][P][128] | dZ [3][4][P][128]), the four upstream gradients (B, out, N) in kernel head order, and
    the float64 parameter gradients laid out as chore_heads_wgrad_floats documents; kept on the device between the tests"""
    if (B, N, kind) not in _HEADS:
        if any(k[:2] != (B, N) for k in _HEADS):
            _HEADS.clear()       # one point count resident at a time: the largest staging is 111 MB
        P = B * N
        rng = _rng("heads", B, N, kind)
        if kind == "random":
            X = rng.standard_normal((P, KPAD), dtype=np.float32)
            Hh = np.maximum(rng.standard_normal((3, 4, P, HID), dtype=np.float32), 0)         # ReLU outputs
            dZ = rng.standard_normal((3, 4, P, HID), dtype=np.float32)
            g = [rng.standard_normal((B, od, N), dtype=np.float32) for od in HEAD_OUT]
        else:
            X = rng.integers(-1, 2, (P, KPAD)).astype(np.float32)
            Hh = rng.integers(-1, 2, (3, 4, P, HID)).astype(np.float32)
            dZ = rng.integers(-1, 2, (3, 4, P, HID)).astype(np.float32)
            g = [rng.integers(-1, 2, (B, od, N)).astype(np.float32) for od in HEAD_OUT]
        X[:, KIN:] = 0           # the pad columns, as the producer leaves them
        t = torch.from_numpy
        X64, H64, Z64 = t(X).double(), t(Hh).double(), t(dZ).double()
        parts = []
        for k, od in enumerate(HEAD_OUT):
            gk = t(g[k]).double().permute(0, 2, 1).reshape(P, od)          # row p = b * N + n
            parts += [Z64[0, k].T @ X64[:, :KIN], Z64[0, k].sum(0), Z64[1, k].T @ H64[0, k], Z64[1, k].sum(0),
                      Z64[2, k].T @ H64[1, k], Z64[2, k].sum(0), gk.T @ H64[2, k], gk.sum(0)]
        names = ["%s.%s" % (hn, pn) for hn in ("df", "parts", "pca", "centers") for pn in ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4")]
        sizes = [p.numel() for p in parts]
        ref = torch.cat([p.reshape(-1) for p in parts]).numpy()
        dev = torch.device("cuda", 0)
        staging = torch.cat([t(X).reshape(-1), t(Hh).reshape(-1), t(dZ).reshape(-1)]).to(dev)
        _HEADS[(B, N, kind)] = (staging, [t(a).to(dev) for a in g], ref, names, sizes)
    return _HEADS[(B, N, kind)]


def _heads_run(B, N, staging, g, flags, prefill, scale=1.0):
    _lib, L, h, dev, stream = _env()
    P, nf = B * N, L.chore_heads_wgrad_floats()
    assert staging.numel() == P * (KPAD + 6 * 4 * HID)
    if scale != 1.0:             # the gradients at another magnitude: dZ (the last third of the staging) and the upstream gradients
        staging = staging.clone()
        staging[P * (KPAD + 3 * 4 * HID):] *= scale
        g = [a * scale for a in g]
    out = Guarded(nf, dev)
    if prefill is not None:
        out.buf[out.m:out.m + nf] = prefill
    ws = Workspace(L.chore_heads_wgrad_workspace_bytes(), dev)
    # argument order of the entry point: df, pca, parts, centers
    _lib.check(L.chore_heads_wgrad(h, staging.data_ptr(), B, N, g[0].data_ptr(), g[2].data_ptr(), g[1].data_ptr(), g[3].data_ptr(), out.ptr,
                                   ws.ptr, flags, stream), h, "heads_wgrad")
    torch.cuda.synchronize()
    ws.check("heads_wgrad")
    return out.read("the gradient arena")


# P = 1, 33, 831 | 833 (26 shares x 32 rows), 1665 (26 x 64 rows: one chunk per share of the fp16 x 3 kernel, and one more), 8193 (128 x
# 64 rows: heads_out_wgrad_kernel wraps); B > 1: the p / N indexing of the output-layer kernel
@pytest.mark.parametrize("B,N", [(1, 1), (1, 33), (3, 277), (1, 833), (3, 555), (3, 2731)])
@pytest.mark.parametrize("x3", [0, 1], ids=["fp32", "x3"])
def test_heads_wgrad(B, N, x3):
    _lib, L, h, dev, stream = _env()
    nf = L.chore_heads_wgrad_floats()
    assert nf == sum(HID * KIN + HID + 2 * (HID * HID + HID) + od * HID + od for od in HEAD_OUT)
    pre = torch.from_numpy(_rng("prefill").integers(-3, 4, nf).astype(np.float32)).to(dev)
    for kind in ("random", "exact"):
        staging, g, ref, names, sizes = _heads_case(B, N, kind)
        for acc in (0, 1):
            for scale in ((1.0, 1e-7, 3e5) if (x3 and kind == "random" and not acc) else (1.0,)):
                got = _heads_run(B, N, staging, g, x3 | (acc << 1), pre if acc else None, scale)
                want = ref * scale + (pre.double().cpu().numpy() if acc else 0.0)
                what = "heads_wgrad%s P %d (B %d) %s acc %d scale %g" % ("_x3" if x3 else "", B * N, B, kind, acc, scale)
                assert np.isfinite(got).all(), what
                if kind == "exact":
                    _exact(got, want, what)
                    continue
                o = 0
                for name, n in zip(names, sizes):        # each tensor against its own largest entry
                    if acc:      # (the bound is on the sum the call adds, not on what the arena held)
                        _close(got[o:o + n] - pre[o:o + n].double().cpu().numpy(), ref[o:o + n] * scale, what + " " + name, HEADS_BOUND)
                    else:
                        _close(got[o:o + n], want[o:o + n], what + " " + name, HEADS_BOUND)
                    o += n
