"""GPU: the 2x2 average pooling of the encoder folded into the producing convolution's epilogue (ConvArgs::pool, csrc/conv_mw.hip), the
statistics stem_x3_kernel accumulates of its own output, and the encoder program built on both (csrc/encoder.hip).

  * single layers through chore_conv2d_pool_fwd, fp16 x 3: y must equal chore_conv2d_fwd's (plus the residual) BIT FOR BIT, y_pool must equal
    chore_avgpool2_fwd(y) bit for bit (the epilogue forms (((a + b) + c) + d) * 0.25f from the stored values in the pass's order; for 32
    channels, which the pass has no instantiation for, the same expression in torch), and the pooled statistics -- reduced from other
    partial sums than the pass's -- agree to 2e-6 of the largest entry, the bound of tests/test_gpu_conv_mw.py.  With y = NULL only the
    pooled tensor is written.  The tiling is an environment switch read once per process (CHORE_CONV_MW_FILL), so each set of cases runs
    in a process of its own; every case reports which kernel its launch reached (chore_debug_last_conv) and the five tilings of the
    production encoder must all have been hit with the pooled output;
  * the 1x1 layer 256 -> 256 (conv_rw_kernel, the merged ml<i> layer that writes `previous`), with and without residual, at 16 x 32,
    16 x 64 and 16 x 40: conv_rw_kernel carries no pooled output (a variant that did measured no gain in the step and slowed the other
    1x1 layers, DESIGN section 4, profiles/r07_pool_fold.txt), so launch_conv refuses it there and the entry point runs the pooling
    pass behind the convolution -- the same y, y_pool and statistics;
  * the whole encoder, default against CHORE_ENC_NO_POOL_FOLD=1 (every pooling pass and every statistic as before): normx and tmpx bit
    for bit, every feature map within the summation-order bound of tests/test_gpu_conv_rw.py (5e-6 of the largest entry), and not all equal;
  * the stem's statistics against chore_gn_stats of its output."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conv_ref import stat_values

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (taps, Cin, Cout, B, H, W): the smallest maps that reach each tiling (conv_mw_tile), whole and -- where the plan allows it: the
# eight-row tiles -- ending inside a tile in both directions with even H and W.  The four-row tiles of 64 and 128 channels come from
# the dense plan only, which takes whole maps (H % 4 == 0, W % 32 == 0)
CASES_256 = [  # CHORE_CONV_MW_FILL=256, a tile per CU: conv_pc_tile's tilings
    (9, 256, 128, 2, 40, 56),     # too few tiles for the wide tilings: 4 x 32 x 32 (not one of the five; pools all the same), ragged
    (9, 128, 64, 3, 20, 28),
    (9, 64, 64, 3, 20, 28),
    (9, 32, 32, 2, 24, 40),
    (9, 32, 128, 8, 64, 128),     # 8 x 32 x 128, whole: 8 * 8 * 4 = 256 tiles
    (9, 32, 64, 8, 64, 128),      # 8 x 32 x 64, whole
    (9, 32, 32, 8, 64, 128),      # 8 x 32 x 32, whole
    (9, 32, 128, 26, 36, 72),     # 8 x 32 x 128, 4.5 x 2.25 tiles per image (26 * 5 * 2 = 260 counted tiles)
    (9, 32, 64, 26, 36, 72),      # 8 x 32 x 64, ragged
    (9, 32, 32, 26, 36, 72),      # 8 x 32 x 32, ragged
]
CASES_DENSE = [  # CHORE_CONV_MW_FILL=16: the widest tile that yields 16 workgroups (the dense tiles of the inference encoder)
    (9, 32, 128, 2, 32, 64),      # 8 x 32 x 128: 2 * 4 * 2 = 16
    (9, 32, 128, 2, 16, 64),      # 4 x 32 x 128: eight rows give 8 workgroups, four rows 16
    (9, 64, 64, 2, 16, 32),       # 2 x 32 x 64 (not one of the five)
    (9, 256, 128, 2, 40, 56),     # W not a multiple of 32: conv_pc_tile's tiling, ragged
    (9, 32, 64, 4, 16, 32),       # 4 x 32 x 64: 4 * 4 * 1 = 16
    (9, 64, 64, 4, 16, 32),       # 4 x 32 x 64, two chunks
]
CASES_RW = [  # 1x1: conv_rw_kernel, no pooled output in its epilogue -> the pooling pass behind the convolution
    (1, 256, 256, 2, 16, 32),
    (1, 256, 256, 2, 16, 64),
    (1, 256, 256, 2, 16, 40),
]

LAYERS = r"""
import sys, ctypes, numpy as np, torch
sys.path.insert(0, {repo!r})
from chore_amd import _lib
L = _lib.lib
dev = torch.device("cuda", 0); h = _lib.handle(0); dt = _lib.F16X3
stream = torch.cuda.current_stream().cuda_stream
out = {{}}
def last():
    rec = (ctypes.c_int * 8)()
    assert L.chore_debug_last_conv(h, rec, 8) == 8
    return np.array(list(rec), np.int64)
def zst(B):
    return torch.zeros(L.chore_gn_stats_bytes(B), dtype=torch.uint8, device=dev)
for n, (taps, cin, cout, B, H, W) in enumerate({cases!r}):
    g = torch.Generator(device=dev); g.manual_seed(300 + n)
    x = torch.randn(B, H, W, cin, device=dev, generator=g) * 1.5 + 0.3
    k = 3 if taps == 9 else 1
    w = torch.randn(cout, cin, k, k, device=dev, generator=g) * (1.0 / np.sqrt(cin * taps))
    ga, be = torch.rand(cin, device=dev, generator=g) + 0.5, torch.randn(cin, device=dev, generator=g) * 0.2
    bias = torch.randn(cout, device=dev, generator=g) * 0.1
    res = torch.randn(B, H, W, cout, device=dev, generator=g)
    st = zst(B)
    _lib.check(L.chore_gn_stats(h, _lib.F32, x.data_ptr(), B, H * W, cin, st.data_ptr(), 1, stream), h, "stats")
    ws = torch.empty(max(16, L.chore_conv2d_workspace_bytes(dt, taps, cin, cout)), dtype=torch.uint8, device=dev)
    # the reference: the convolution alone, the residual added in torch (one fp32 add per element, as the epilogue's), the pooling pass
    y0 = torch.full((B, H, W, cout), 7.0, device=dev)
    _lib.check(L.chore_conv2d_fwd(h, dt, taps, x.data_ptr(), B, H, W, cin, st.data_ptr(), ga.data_ptr(), be.data_ptr(), w.data_ptr(),
                                  bias.data_ptr(), cout, y0.data_ptr(), None, ws.data_ptr(), stream), h, "conv")
    for tag, r in (("n", None), ("r", res)):
        want = y0 if r is None else y0 + r
        # (((a + b) + c) + d) * 0.25f, PoolOp::column's order; each torch op is one correctly rounded fp32 operation
        pw = (((want[:, 0::2, 0::2] + want[:, 0::2, 1::2]) + want[:, 1::2, 0::2]) + want[:, 1::2, 1::2]) * 0.25
        stp = zst(B)
        if cout in (64, 128, 256):
            pp = torch.full((B, H // 2, W // 2, cout), 5.0, device=dev)
            _lib.check(L.chore_avgpool2_fwd(h, _lib.F32, want.contiguous().data_ptr(), pp.data_ptr(), B, H, W, cout, stp.data_ptr(), stream), h, "pool")
            torch.cuda.synchronize()
            assert torch.equal(pp, pw), "the pooling pass and its torch transcription disagree"
        else:
            _lib.check(L.chore_gn_stats(h, _lib.F32, pw.contiguous().data_ptr(), B, (H // 2) * (W // 2), cout, stp.data_ptr(), 1, stream), h, "stats")
        for ytag, with_y in (("y", True), ("o", False)):
            if not with_y and taps == 1:
                continue                       # the pass needs y
            y = torch.full((B, H, W, cout), 7.0, device=dev)
            # y_pool sits between two guard bands: nothing but the pooled tensor may be written (y = NULL writes nothing else at all)
            npool, G = B * (H // 2) * (W // 2) * cout, 4096
            ypbuf = torch.full((npool + 2 * G,), 3.0, device=dev)
            yp = ypbuf[G:G + npool].view(B, H // 2, W // 2, cout)
            sy, sp = zst(B), zst(B)
            _lib.check(L.chore_conv2d_pool_fwd(h, dt, taps, x.data_ptr(), B, H, W, cin, st.data_ptr(), ga.data_ptr(), be.data_ptr(),
                                               w.data_ptr(), bias.data_ptr(), cout, None if r is None else r.data_ptr(),
                                               y.data_ptr() if with_y else None, sy.data_ptr() if with_y else None, yp.data_ptr(),
                                               sp.data_ptr(), ws.data_ptr(), stream), h, "conv_pool")
            rec = last()
            torch.cuda.synchronize()
            key = "%d%s%s" % (n, tag, ytag)
            out["rec" + key] = rec
            out["y_eq" + key] = np.array(bool(torch.equal(y, want)) if with_y else True)
            out["p_eq" + key] = np.array(bool(torch.equal(yp, pw)) and bool((ypbuf[:G] == 3.0).all()) and bool((ypbuf[G + npool:] == 3.0).all()))
            out["p_max" + key] = np.array(float(yp.abs().max()))
            out["sp" + key] = sp.cpu().numpy().view(np.int64)
            out["sp_ref" + key] = stp.cpu().numpy().view(np.int64)
            if with_y:
                sref = zst(B)
                _lib.check(L.chore_gn_stats(h, _lib.F32, want.contiguous().data_ptr(), B, H * W, cout, sref.data_ptr(), 1, stream), h, "stats")
                torch.cuda.synchronize()
                out["sy" + key] = sy.cpu().numpy().view(np.int64)
                out["sy_ref" + key] = sref.cpu().numpy().view(np.int64)
np.savez({path!r}, **out)
"""

ENCODER = r"""
import sys, numpy as np, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {repo!r} + "/tests")
from bench import chore_opt
from chore_amd.model import CHORE
from chore_amd.utils import synth
net = CHORE(chore_opt("fp16x3")).cuda().eval(); synth.load_synth_weights(net, 0)
for p in net.parameters(): p.requires_grad_(False)
img = torch.from_numpy(synth.synth_images({B}, {H}, {W}, 5)).cuda()
with torch.no_grad():
    net.filter(img)
out = dict(("f%d" % i, o.float().cpu().numpy()) for i, o in enumerate(net.im_feat_list))
out["tmpx"] = net.tmpx.float().cpu().numpy(); out["normx"] = net.normx.float().cpu().numpy()
np.savez({path!r}, **out)
"""

STEM = r"""
import sys, numpy as np, torch
sys.path.insert(0, {repo!r})
from chore_amd import _lib
L = _lib.lib
dev = torch.device("cuda", 0); h = _lib.handle(0)
stream = torch.cuda.current_stream().cuda_stream
B, Cin, H, W = 2, 5, 64, 96
g = torch.Generator(device=dev); g.manual_seed(7)
img = torch.rand(B, Cin, H, W, device=dev, generator=g)
w = torch.randn(64, Cin, 7, 7, device=dev, generator=g) * 0.1
bias = torch.randn(64, device=dev, generator=g) * 0.1
y = torch.zeros(B, H // 2, W // 2, 64, device=dev)
ws = torch.empty(L.chore_stem_x3_workspace_bytes(Cin), dtype=torch.uint8, device=dev)
st = torch.zeros(L.chore_gn_stats_bytes(B), dtype=torch.uint8, device=dev)
_lib.check(L.chore_stem_x3_fwd(h, img.data_ptr(), B, Cin, H, W, w.data_ptr(), bias.data_ptr(), y.data_ptr(), st.data_ptr(), ws.data_ptr(), stream), h, "stem")
ref = torch.zeros_like(st)
_lib.check(L.chore_gn_stats(h, _lib.F32, y.data_ptr(), B, (H // 2) * (W // 2), 64, ref.data_ptr(), 1, stream), h, "stats")
torch.cuda.synchronize()
np.savez({path!r}, y=y.cpu().numpy(), st=st.cpu().numpy().view(np.int64), ref=ref.cpu().numpy().view(np.int64))
"""


def run(tmp_path, script, tag, env, **kw):
    path = str(tmp_path / ("pf_%s.npz" % tag))
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", script.format(repo=REPO, path=path, **kw)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(path))


def check_layers(d, cases, want_fold):
    """every case of one process; want_fold(case) -> the launch must have carried the pooled output.  Returns the (rows, nt, tps,
    nslot) tilings of conv_mw_kernel that did"""
    hit = set()
    for n, (taps, cin, cout, B, H, W) in enumerate(cases):
        for tag in "nr":
            for ytag in ("y", "o") if taps == 9 else ("y",):
                key = "%d%s%s" % (n, tag, ytag)
                case = (taps, cin, cout, B, H, W, tag, ytag)
                rec = d["rec" + key]
                assert bool(d["y_eq" + key]), ("y", case)
                assert bool(d["p_eq" + key]) and float(d["p_max" + key]) > 0.05, ("y_pool", case)
                sp, ref = stat_values(d["sp" + key]), stat_values(d["sp_ref" + key])
                print("pool stats", case, "deviation %.2e of %.3e" % (np.abs(sp - ref).max(), np.abs(ref).max()))
                assert np.abs(sp - ref).max() <= 2e-6 * np.abs(ref).max(), ("pool_stats", case, np.abs(sp - ref).max(), np.abs(ref).max())
                if ytag == "y":
                    sy, ref = stat_values(d["sy" + key]), stat_values(d["sy_ref" + key])
                    assert np.abs(sy - ref).max() <= 2e-6 * np.abs(ref).max(), ("out_stats", case, np.abs(sy - ref).max(), np.abs(ref).max())
                folded = bool(rec[5] & 16)
                assert folded == want_fold(cases[n]), (case, list(rec))
                assert bool(rec[5] & 8) == (tag == "r"), (case, list(rec))
                assert rec[0] == (4 if taps == 9 else 5), (case, list(rec))      # conv_mw_kernel / conv_rw_kernel
                if folded and taps == 9:
                    hit.add(tuple(int(v) for v in rec[1:5]))
    return hit


FIVE = {(8, 128, 1, 3), (8, 64, 3, 2), (8, 32, 3, 2), (4, 128, 1, 3), (4, 64, 3, 2)}


def test_layers_pool_in_the_epilogue_bit_for_bit(tmp_path):
    a = run(tmp_path, LAYERS, "l256", {"CHORE_CONV_MW_FILL": "256"}, cases=CASES_256)
    b = run(tmp_path, LAYERS, "l16", {"CHORE_CONV_MW_FILL": "16"}, cases=CASES_DENSE)
    hit = check_layers(a, CASES_256, lambda c: True) | check_layers(b, CASES_DENSE, lambda c: True)
    print("tilings that carried a pooled output:", sorted(hit))
    assert FIVE <= hit, sorted(FIVE - hit)


def test_1x1_layers_fall_back_to_the_pooling_pass(tmp_path):
    d = run(tmp_path, LAYERS, "rw", {}, cases=CASES_RW)
    check_layers(d, CASES_RW, lambda c: False)


def test_encoder_with_folded_pooling_equals_encoder_with_passes(tmp_path):
    a = run(tmp_path, ENCODER, "enc_fold", {}, B=3, H=80, W=112)
    b = run(tmp_path, ENCODER, "enc_pass", {"CHORE_ENC_NO_POOL_FOLD": "1"}, B=3, H=80, W=112)
    assert set(a) == set(b) and len(a) >= 3
    for k in ("normx", "tmpx"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    worst = 0.0
    for k in a:
        assert np.isfinite(a[k]).all()
        err = np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()
        worst = max(worst, err)
        assert err <= 5e-6, (k, err)
    print("folded pooling vs passes, encoder 3x80x112: worst relative deviation %.2e" % worst)
    assert any((a[k] != b[k]).any() for k in a)      # the switch did something


def test_stem_statistics_equal_a_pass_over_its_output(tmp_path):
    d = run(tmp_path, STEM, "stem", {})
    assert np.isfinite(d["y"]).all() and np.abs(d["y"]).max() > 0.1
    st, ref = stat_values(d["st"]), stat_values(d["ref"])
    print("stem statistics: deviation %.2e of %.3e" % (np.abs(st - ref).max(), np.abs(ref).max()))
    assert np.abs(st - ref).max() <= 2e-6 * np.abs(ref).max()
