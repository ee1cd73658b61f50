"""GPU: the encoder's map operators -- csrc/enc_misc.hip behind the entry points of csrc/ops.hip: chore_gn_stats, chore_gn_relu_fwd,
chore_avgpool2_fwd / _bwd, chore_upadd_fwd, chore_up2_bwd, chore_stem_fwd, chore_stem_x3_fwd, chore_absmax_f32 -- called directly
through the C API at every case of tests/map_cases.py and compared with the float64 references of tests/map_ref.py.

Outputs live between sentinel margins and are pre-filled with NaN; workspaces and statistics accumulators have exactly the size
their *_bytes function states, plus a sentinel page (tests/gpu_guards.py).

Bounds (none tuned to the device).
  exact kind     bit for bit, values and statistics (map_cases.py says what "exact" is for each family).
  fp32 values    within F32_BOUND = 2e-5 of the reference's largest entry (test_gpu_train_ops.py, test_gpu_bwd_operators.py).
  16-bit values  the reference is fed the rounded inputs; per element |got - ref| <= ulp(ref) + 2e-5 of the largest entry, ulp = 2^-7
                 (bf16) or 2^-10 (f16) of |ref|: the float64 value and the device's fp32 value may round to opposite sides of a tie.
  statistics     against the float64 sums of the values as stored (the device's own output, read back):
                 (L + P + gs) 2^-24 sum |v| + n 2^-40 for the sum, the same with sum v^2 for the squares -- L the longest per-thread
                 chain, P the partials a channel's reducer adds, gs = C / 32 the lanes of a group, n the atomic adds into the cell
                 (stat_add drops what lies below the unit 2^-40 of the fixed-point accumulator; the accumulation itself is exact).
  stem_x3        per element 2^-22 (|w| * |x|) + (49 Cin + 1) 2^-24 (|w| * |x|): the dropped lo x lo term and the fp32 sums.
  absmax         the maximum over the cells, as float bits, equals the reference's.
  adjointness    <U low, dy> from chore_upadd_fwd (a = 0) and <low, U^T dy> from chore_up2_bwd, summed in float64 on the host, agree to
                 2e-5 of the sum of the terms' magnitudes.

Measured on an MI355X (worst error over the cases, next to its bound; the module's 607 tests take 5 s):
  chore_gn_relu_fwd    fp32 1.4e-07 (2e-5); bf16 0.50 and f16 0.48 of the per-element bound: the half ulp of the device's own rounding
  chore_avgpool2_fwd   fp32 8.5e-08 (2e-5); bf16 0.50 of its bound -- no bf16 case beyond one ulp;  _bwd  exact in every case, random kind too
  chore_upadd_fwd      fp32 9.2e-06 (2e-5) at 255 x 2, 4.0e-06 at 3 x 128, 8.6e-07 at 12 x 17: the source coordinate is an fp32 product that
                       grows with the axis, as in ATen's kernel; bf16 0.50, f16 0.48 of their bounds
  chore_up2_bwd        fp32 9.0e-06 (2e-5) at 255 x 2, 1.1e-06 up to n = 20; bf16 0.49 of its bound
  adjointness          3.0e-09 of the sum of the terms' magnitudes (2e-5)
  chore_stem_fwd       fp32 8.8e-07 (2e-5) at Cin = 8; bf16 0.49 of its bound
  chore_stem_x3_fwd    0.16 of the per-element bound
  statistics           share of the bound used, sum / squares: chore_gn_stats 0.09 / 0.15, pooling 0.07 / 0.11, up-add 0.04 / 0.09,
                       stem_x3 0.03 / 0.06 -- the bounds are worst-case chains, so the exact-kind twin of every shape is the sharp check
  chore_absmax_f32     the tensor's bits in every case
  every exact case came out bit for bit, every guard margin, workspace page and accumulator page held, every row of the refused
  family was refused with its outputs, statistics and workspace untouched.
Libraries with one slip each failed where they should: the last output row left out of map_stats_kernel's statistics fails all
96 pool and all 42 upadd cases; act_hi_cells(1) for act_hi_cells(gridDim.y) every case with B = 3 (48 gn_stats, 48 pool, 20 upadd,
3 gn_relu); the tail loop of absmax_block one stride late 16 absmax cases (every one whose maximum sits in the first vector of a thread's tail).
UpAddOp::PSX one smaller does not compile: the static_assert on the tile geometry.  The window of up2_bwd_kernel started at
2 l - 4 instead of 2 l - 5 fails nothing and cannot: no coordinate below 2 l - 3 weighs on l (test_map_coverage_table.py asserts
it), the result is the same; started at 2 l - 2 (rows only) it fails the 49 random-kind up2_bwd cases with H >= 3
and two of the three adjointness cases.
"""
import numpy as np
import pytest
import torch

import map_cases as mc
import map_ref as mr
from gpu_guards import WORST, Guarded, Workspace, _close, _exact

pytestmark = pytest.mark.gpu

F32_BOUND = 2e-5
U24 = 2.0 ** -24
EINVAL = -1


def _env():
    from chore_amd import _lib
    dev = torch.device("cuda", 0)
    return _lib, _lib.lib, _lib.handle(0), dev, torch.cuda.current_stream(dev).cuda_stream


def _dt(_lib, dtype):
    return {"f32": _lib.F32, "bf16": _lib.BF16, "f16": _lib.F16}.get(dtype, dtype)


def _note(tag, err, bound, what):
    if err > WORST.get(tag, (-1.0,))[0]:
        WORST[tag] = (err, 0.0, what)
        print("  worst so far %-26s %.2e (bound %.1e)   at %s" % (tag, err, bound, what))


def _cmp(got, ref, what, dtype):
    """fp32: within F32_BOUND of the largest entry; 16-bit storage: one unit in the last place of the reference more"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if dtype == "f32":
        return _close(got, ref, what, F32_BOUND)
    assert np.isfinite(got).all(), "%s: %d entries not written or not finite" % (what, int((~np.isfinite(got)).sum()))
    top = np.abs(ref).max()
    assert top > 0, what
    err, bound = np.abs(got - ref), mr.ULP[dtype] * np.abs(ref) + F32_BOUND * top
    k = np.unravel_index((err / bound).argmax(), ref.shape)
    _note(what.split(" ")[0] + " " + dtype, float(err[k] / bound[k]), 1.0, what)
    assert err[k] <= bound[k], "%s: |%r - %r| = %.3e at %s, bound %.3e (one %s ulp and %.0e of %.3g)" % (
        what, float(got[k]), float(ref[k]), err[k], k, bound[k], dtype, F32_BOUND, top)


def _exact_dyadic(got, ref, what, unit=1):
    """bit for bit; `unit`: the power of two that makes every reference value an integer"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: %d entries not written or not finite" % (what, int((~np.isfinite(got)).sum()))
    _exact(got * unit, ref * unit, what)


def _stats(st, B, stored64, chain, adds, kind, what, unit=1):
    """the accumulators against the float64 sums of the values as stored"""
    st.check(what)
    s, q = mr.stats_decode(st.buf[:st.nbytes], B)
    rs, rq, ra = mr.group_stats(stored64)
    if kind == "exact":
        _exact_dyadic(s, rs, what + " sum", unit)
        _exact_dyadic(q, rq, what + " sq", unit * unit)
        return
    L, P = chain
    gs = stored64.shape[-1] // mr.GROUPS
    for name, got, ref, mag in (("sum", s, rs, ra), ("sq", q, rq, rq)):
        bound = (L + P + gs) * U24 * mag + adds * 2.0 ** -40
        err = np.abs(got - ref)
        k = np.unravel_index((err / bound).argmax(), ref.shape)
        _note(what.split(" ")[0] + " " + name, float(err[k] / bound[k]), 1.0, what)
        assert (err <= bound).all(), "%s %s: |%r - %r| = %.3e at (image, group) %s, bound %.3e = (%d + %d + %d) 2^-24 %.6g" % (
            what, name, float(got[k]), float(ref[k]), err[k], k, bound[k], L, P, gs, mag[k])


def _stat_buffer(L, B, dev, zero=True):
    return Workspace(L.chore_gn_stats_bytes(B), dev, zero=zero)


def _ptr(t):
    return None if t is None else t.ptr


# ================================================================================================ chore_gn_stats
@pytest.mark.parametrize("case", mc.CASES["gn_stats"], ids=mc.ids("gn_stats"))
def test_gn_stats(case):
    _lib, L, h, dev, stream = _env()
    B, HW, C, dtype = case["B"], case["HW"], case["C"], case["dtype"]
    xs = mr.stored(mc.values(case, (B, HW, C)), dtype)
    xd, x64 = xs.to(dev), xs.double().numpy()
    chain_L, chain_P, adds = mc.gn_stats_chain(C, HW)
    for zeroed in (0, 1):          # 0: the entry point clears accumulators full of garbage itself; 1: the caller hands it zeros
        st = _stat_buffer(L, B, dev, zero=bool(zeroed))
        _lib.check(L.chore_gn_stats(h, _dt(_lib, dtype), xd.data_ptr(), B, HW, C, st.ptr, zeroed, stream), h, "gn_stats")
        torch.cuda.synchronize()
        _stats(st, B, x64, (chain_L, chain_P), adds, case["kind"], "gn_stats %s zeroed %d" % (case["id"], zeroed))


# ================================================================================================ chore_gn_relu_fwd
@pytest.mark.parametrize("case", mc.CASES["gn_relu"], ids=mc.ids("gn_relu"))
def test_gn_relu(case):
    _lib, L, h, dev, stream = _env()
    B, HW, C, dtype = case["B"], case["HW"], case["C"], case["dtype"]
    xs = mr.stored(mc.values(case, (B, HW, C)), dtype)
    xd, x64 = xs.to(dev), xs.double().numpy()
    gamma, beta = mc.gn_relu_affine(case)
    gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    st = _stat_buffer(L, B, dev)
    if case["stats"] == "device":
        _lib.check(L.chore_gn_stats(h, _dt(_lib, dtype), xd.data_ptr(), B, HW, C, st.ptr, 1, stream), h, "gn_stats")
    else:          # the float64 statistics of the stored input: this operator's verdict does not depend on chore_gn_stats
        rs, rq, _ = mr.group_stats(x64)
        st.buf[:st.nbytes] = torch.from_numpy(mr.stats_encode(rs, rq)).to(dev)
    y = Guarded(B * HW * C, dev, mr.TORCH_DTYPE[dtype])
    _lib.check(L.chore_gn_relu_fwd(h, _dt(_lib, dtype), xd.data_ptr(), st.ptr, gd.data_ptr(), bd.data_ptr(), y.ptr, B, HW, C, stream), h, "gn_relu_fwd")
    torch.cuda.synchronize()
    st.check("gn_relu_fwd")
    got = y.read(case["id"]).reshape(B, HW, C)
    if case["kind"] == "exact":
        _exact_dyadic(got, np.broadcast_to(np.maximum(beta.astype(np.float64), 0.0), got.shape), "gn_relu " + case["id"])
    else:
        _cmp(got, mr.gn_relu(x64, gamma.astype(np.float64), beta.astype(np.float64)), "gn_relu " + case["id"], dtype)


# ================================================================================================ chore_avgpool2_fwd / _bwd
def _tiles(OH, OW, TW):
    return -(-OH // mc.CONSTANTS["MAP_T"]) * -(-OW // TW)


@pytest.mark.parametrize("case", mc.CASES["pool"], ids=mc.ids("pool"))
def test_pool(case):
    _lib, L, h, dev, stream = _env()
    B, H, W, C, dtype = case["B"], case["H"], case["W"], case["C"], case["dtype"]
    xs = mr.stored(mc.values(case, (B, H, W, C)), dtype)
    xd, ref = xs.to(dev), mr.avgpool2(xs.double().numpy())
    for with_stats in (True, False):
        what = "pool %s%s" % (case["id"], "" if with_stats else " no statistics")
        y = Guarded(ref.size, dev, mr.TORCH_DTYPE[dtype])
        st = _stat_buffer(L, B, dev) if with_stats else None
        _lib.check(L.chore_avgpool2_fwd(h, _dt(_lib, dtype), xd.data_ptr(), y.ptr, B, H, W, C, _ptr(st), stream), h, "avgpool2_fwd")
        torch.cuda.synchronize()
        got = y.read(what).reshape(ref.shape)
        if case["kind"] == "exact":
            _exact_dyadic(got, ref, what, 4)
        else:
            _cmp(got, ref, what, dtype)
        if st is not None:
            _stats(st, B, got, mc.map_chain(C, C, mc.CONSTANTS["MAP_T"]), _tiles(H // 2, W // 2, mc.CONSTANTS["MAP_T"]), case["kind"], "pool.stats " + case["id"], 4)


@pytest.mark.parametrize("case", mc.CASES["pool_bwd"], ids=mc.ids("pool_bwd"))
def test_pool_bwd(case):
    _lib, L, h, dev, stream = _env()
    B, H, W, C, dtype = case["B"], case["H"], case["W"], case["C"], case["dtype"]
    dys = mr.stored(mc.values(case, (B, H // 2, W // 2, C)), dtype)
    dyd, ref = dys.to(dev), mr.avgpool2_bwd(dys.double().numpy())
    dx = Guarded(ref.size, dev, mr.TORCH_DTYPE[dtype])
    _lib.check(L.chore_avgpool2_bwd(h, _dt(_lib, dtype), dyd.data_ptr(), dx.ptr, B, H, W, C, stream), h, "avgpool2_bwd")
    torch.cuda.synchronize()
    got = dx.read(case["id"]).reshape(ref.shape)
    if case["kind"] == "exact":
        _exact_dyadic(got, ref, "pool_bwd " + case["id"], 4)
    else:
        _cmp(got, ref, "pool_bwd " + case["id"], dtype)


# ================================================================================================ chore_upadd_fwd
@pytest.mark.parametrize("case", mc.CASES["upadd"], ids=mc.ids("upadd"))
def test_upadd(case):
    _lib, L, h, dev, stream = _env()
    B, H, W, C, dtype = case["B"], case["H"], case["W"], case["C"], case["dtype"]
    a, low = (mr.stored(t, dtype) for t in mc.upadd_inputs(case))
    ad, lowd = a.to(dev), low.to(dev)
    ref = mr.upadd(a.double().numpy(), low.double().numpy())
    for with_stats in (True, False):
        what = "upadd %s%s" % (case["id"], "" if with_stats else " no statistics")
        y = Guarded(ref.size, dev, mr.TORCH_DTYPE[dtype])
        st = _stat_buffer(L, B, dev) if with_stats else None
        a_ptr = ad.data_ptr()
        if case["inplace"]:          # y is a: every element is read and written by the same thread
            y.buf[y.m:y.m + y.n] = ad.reshape(-1)
            a_ptr = y.ptr
        _lib.check(L.chore_upadd_fwd(h, _dt(_lib, dtype), a_ptr, lowd.data_ptr(), y.ptr, B, H, W, C, _ptr(st), stream), h, "upadd_fwd")
        torch.cuda.synchronize()
        got = y.read(what).reshape(ref.shape)
        if case["kind"] == "exact":
            _exact_dyadic(got, ref, what)
        else:
            _cmp(got, ref, what, dtype)
        if st is not None:
            _stats(st, B, got, mc.map_chain(C, mc.CONSTANTS["UP_CT"], mc.CONSTANTS["UP_TW"]), _tiles(2 * H, 2 * W, mc.CONSTANTS["UP_TW"]),
                   case["kind"], "upadd.stats " + case["id"])


# ================================================================================================ chore_up2_bwd
def _up2_bwd_run(dy, B, H, W, C, dtype, what):
    _lib, L, h, dev, stream = _env()
    dyd = dy.to(dev)
    dlow = Guarded(B * H * W * C, dev, mr.TORCH_DTYPE[dtype])
    _lib.check(L.chore_up2_bwd(h, _dt(_lib, dtype), dyd.data_ptr(), dlow.ptr, B, H, W, C, stream), h, "up2_bwd")
    torch.cuda.synchronize()
    return dlow.read(what).reshape(B, H, W, C)


@pytest.mark.parametrize("case", mc.CASES["up2_bwd"], ids=mc.ids("up2_bwd"))
def test_up2_bwd(case):
    B, H, W, C, dtype = case["B"], case["H"], case["W"], case["C"], case["dtype"]
    dys = mr.stored(mc.up2_bwd_input(case), dtype)
    ref = mr.up2_bwd(dys.double().numpy())
    got = _up2_bwd_run(dys, B, H, W, C, dtype, case["id"])
    if case["kind"] == "exact":
        _exact_dyadic(got, ref, "up2_bwd " + case["id"])
    else:
        _cmp(got, ref, "up2_bwd " + case["id"], dtype)


@pytest.mark.parametrize("size", mc.ADJOINT_HW, ids=["%dx%d" % s for s in mc.ADJOINT_HW])
def test_upadd_and_up2_bwd_are_adjoint(size):
    _lib, L, h, dev, stream = _env()
    (H, W), B, C = size, 2, 64
    r = mc.rng("adjoint", size)
    low = r.standard_normal((B, H, W, C), dtype=np.float32)
    dy = r.standard_normal((B, 2 * H, 2 * W, C), dtype=np.float32)
    lowd, zero = torch.from_numpy(low).to(dev), torch.zeros(dy.shape, device=dev)
    y = Guarded(dy.size, dev)
    _lib.check(L.chore_upadd_fwd(h, _lib.F32, zero.data_ptr(), lowd.data_ptr(), y.ptr, B, H, W, C, None, stream), h, "upadd_fwd")
    torch.cuda.synchronize()
    up = y.read("adjoint upadd").reshape(dy.shape)
    dlow = _up2_bwd_run(torch.from_numpy(dy), B, H, W, C, "f32", "adjoint up2_bwd")
    terms = up * dy.astype(np.float64)
    lhs, rhs = terms.sum(), (low.astype(np.float64) * dlow).sum()
    _note("adjoint", abs(lhs - rhs) / np.abs(terms).sum(), F32_BOUND, "%dx%d" % size)
    assert abs(lhs - rhs) <= F32_BOUND * np.abs(terms).sum(), (size, lhs, rhs)


# ================================================================================================ chore_stem_fwd / chore_stem_x3_fwd
@pytest.mark.parametrize("case", mc.CASES["stem"], ids=mc.ids("stem"))
def test_stem(case):
    _lib, L, h, dev, stream = _env()
    B, Cin, H, W, dtype = case["B"], case["Cin"], case["H"], case["W"], case["dtype"]
    img, w, bias = mc.stem_inputs(case)
    ref, _ = mr.stem(img, w, bias)
    imgd, wd, bd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (img, w, bias))
    ws = Workspace(L.chore_stem_workspace_bytes(Cin), dev)
    y = Guarded(ref.size, dev, mr.TORCH_DTYPE[dtype])
    _lib.check(L.chore_stem_fwd(h, _dt(_lib, dtype), imgd.data_ptr(), B, Cin, H, W, wd.data_ptr(), bd.data_ptr(), y.ptr, ws.ptr, stream), h, "stem_fwd")
    torch.cuda.synchronize()
    ws.check("stem_fwd")
    got = y.read(case["id"]).reshape(ref.shape)
    if case["kind"] == "exact":
        _exact_dyadic(got, ref, "stem " + case["id"])
    else:
        _cmp(got, ref, "stem " + case["id"], dtype)


@pytest.mark.parametrize("case", mc.CASES["stem_x3"], ids=mc.ids("stem_x3"))
def test_stem_x3(case):
    _lib, L, h, dev, stream = _env()
    B, Cin, H, W = case["B"], case["Cin"], case["H"], case["W"]
    img, w, bias = mc.stem_inputs(case)
    ref, mag = mr.stem(img, w, bias)
    imgd, wd, bd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (img, w, bias))
    for with_stats in (True, False):
        what = "stem_x3 %s%s" % (case["id"], "" if with_stats else " no statistics")
        ws = Workspace(L.chore_stem_x3_workspace_bytes(Cin), dev)
        y = Guarded(ref.size, dev)
        st = _stat_buffer(L, B, dev) if with_stats else None
        _lib.check(L.chore_stem_x3_fwd(h, imgd.data_ptr(), B, Cin, H, W, wd.data_ptr(), bd.data_ptr(), y.ptr, _ptr(st), ws.ptr, stream), h, "stem_x3_fwd")
        torch.cuda.synchronize()
        ws.check("stem_x3_fwd")
        got = y.read(what).reshape(ref.shape)
        if case["kind"] == "exact":
            _exact_dyadic(got, ref, what)
        else:
            assert np.isfinite(got).all(), what
            bound = (2.0 ** -22 + (49 * Cin + 1) * U24) * mag
            err = np.abs(got - ref)
            k = np.unravel_index((err - bound).argmax(), ref.shape)
            _note("stem_x3", float((err / np.maximum(bound, 1e-300)).max()), 1.0, what)
            assert err[k] <= bound[k], "%s: |%r - %r| = %.3e at %s, bound %.3e" % (what, float(got[k]), float(ref[k]), err[k], k, bound[k])
        if st is not None:
            tiles = -(-(H // 2) // mc.CONSTANTS["STEM_T"]) * -(-(W // 2) // mc.CONSTANTS["SX_TW"])
            _stats(st, B, got, mc.STEM_X3_CHAIN, tiles, case["kind"], "stem_x3.stats " + case["id"])


# ================================================================================================ chore_absmax_f32
@pytest.mark.parametrize("case", mc.CASES["absmax"], ids=mc.ids("absmax"))
def test_absmax(case):
    _lib, L, h, dev, stream = _env()
    x = mc.absmax_input(case)
    xd = torch.from_numpy(x).to(dev)
    cells = Workspace(L.chore_amax_bytes(), dev)
    assert cells.nbytes == 4 * mc.CONSTANTS["AMAX_CELLS"]
    _lib.check(L.chore_absmax_f32(h, xd.data_ptr(), x.size, cells.ptr, stream), h, "absmax_f32")
    torch.cuda.synchronize()
    cells.check("absmax_f32")
    got = int(cells.buf[:cells.nbytes].cpu().numpy().view(np.uint32).max())
    want = mr.absmax_bits(x)
    assert got == want, "%s: max |x| came out as bits %08x, the tensor's are %08x (vector %d of %d)" % (case["id"], got, want, case["vec"], x.size // 4)
    if case["special"] == "zero":
        assert got == 0


# ================================================================================================ refusals
# a small valid call of every entry point; a refused case replaces some of its arguments.  Buffers are sized for the largest
# refused shape, so that a call that went through would stay inside them
_REFUSED_BASE = {
    "chore_gn_stats": dict(dtype="f32", B=2, HW=10, C=64),
    "chore_gn_relu_fwd": dict(dtype="f32", B=2, HW=10, C=64),
    "chore_avgpool2_fwd": dict(dtype="f32", B=2, H=4, W=4, C=64),
    "chore_avgpool2_bwd": dict(dtype="f32", B=2, H=4, W=4, C=64),
    "chore_upadd_fwd": dict(dtype="f32", B=2, H=3, W=3, C=64),
    "chore_up2_bwd": dict(dtype="f32", B=2, H=3, W=3, C=8),
    "chore_stem_fwd": dict(dtype="f32", B=1, Cin=3, H=8, W=8),
    "chore_stem_x3_fwd": dict(B=1, Cin=3, H=8, W=8),
    "chore_absmax_f32": dict(n=64, misalign=0, null=False),
}
_ROOM = 1 << 16          # elements of every input and output buffer of a refused call


@pytest.mark.parametrize("case", mc.CASES["refused"], ids=mc.ids("refused"))
def test_refused(case):
    _lib, L, h, dev, stream = _env()
    fn, a = case["fn"], dict(_REFUSED_BASE[case["fn"]], **case["over"])
    dt = _dt(_lib, a.get("dtype"))
    src = [torch.zeros(_ROOM, device=dev) for _ in range(4)]
    p = [t.data_ptr() for t in src]
    out = Guarded(_ROOM, dev, fill=3.0)
    st = _stat_buffer(L, 2, dev, zero=False)          # garbage: a refused call must not even clear it
    ws = Workspace(1 << 20, dev)
    before = [t.buf.clone() for t in (st, ws)]
    if fn == "chore_gn_stats":
        rc = L.chore_gn_stats(h, dt, p[0], a["B"], a["HW"], a["C"], st.ptr, 0, stream)
    elif fn == "chore_gn_relu_fwd":
        rc = L.chore_gn_relu_fwd(h, dt, p[0], st.ptr, p[1], p[2], out.ptr, a["B"], a["HW"], a["C"], stream)
    elif fn == "chore_avgpool2_fwd":
        rc = L.chore_avgpool2_fwd(h, dt, p[0], out.ptr, a["B"], a["H"], a["W"], a["C"], st.ptr, stream)
    elif fn == "chore_avgpool2_bwd":
        rc = L.chore_avgpool2_bwd(h, dt, p[0], out.ptr, a["B"], a["H"], a["W"], a["C"], stream)
    elif fn == "chore_upadd_fwd":
        rc = L.chore_upadd_fwd(h, dt, p[0], p[1], out.ptr, a["B"], a["H"], a["W"], a["C"], st.ptr, stream)
    elif fn == "chore_up2_bwd":
        rc = L.chore_up2_bwd(h, dt, p[0], out.ptr, a["B"], a["H"], a["W"], a["C"], stream)
    elif fn == "chore_stem_fwd":
        assert L.chore_stem_workspace_bytes(a["Cin"]) <= ws.nbytes
        rc = L.chore_stem_fwd(h, dt, p[0], a["B"], a["Cin"], a["H"], a["W"], p[1], p[2], out.ptr, ws.ptr, stream)
    elif fn == "chore_stem_x3_fwd":
        assert L.chore_stem_x3_workspace_bytes(a["Cin"]) <= ws.nbytes
        rc = L.chore_stem_x3_fwd(h, p[0], a["B"], a["Cin"], a["H"], a["W"], p[1], p[2], out.ptr, st.ptr, ws.ptr, stream)
    else:
        assert fn == "chore_absmax_f32"
        rc = L.chore_absmax_f32(h, None if a["null"] else p[0] + a["misalign"], a["n"], ws.ptr, stream)
    torch.cuda.synchronize()
    msg = L.chore_last_error(h).decode()
    assert rc == EINVAL, "%s: returned %d (%s)" % (case["id"], rc, msg)
    assert case["msg"] in msg, (case["id"], msg)
    assert (out.read("refused " + case["id"]) == 3.0).all(), case["id"]
    for t, b, name in zip((st, ws), before, ("statistics", "workspace")):
        assert torch.equal(t.buf.view(torch.int8), b.view(torch.int8)), "%s: the refused call wrote its %s" % (case["id"], name)
