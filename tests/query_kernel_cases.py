"""The cases of tests/test_gpu_query_kernels.py: which calls are made under which switch set, with which inputs, and which bounds hold.
No GPU and no library call in here; tests/test_query_coverage_table.py checks this file on the CPU.

Selection.  From query_plan_cases.CASES (without 4 x 20000, the benchmark's shape): under every switch set, for every distinct
(kernel name, sort) pair the expectations name under that set, the smallest case that reaches it -- fewest points, then the
16 x 16 map, then the list's order.  To these come, under every set, the ragged counts N = 1, 63, 65 of every operation (EXTRA
where the plan file has no such row), a backward with two absent gradients at 2 x 333 (an absent head contributes nothing), every
head of the one-head backward (its kernel name does not say which head runs) and the 32-point fp16 x 3 backward over more than 256
tiles at 4 x 4160.  A staged training backward reads what the training forward of the same inputs wrote, so that forward is a case
of the same set.  EXTRA rows spell their expectation out like the plan file's rows; the coverage test holds them against
chore_query_plan.

Inputs (as scripts/query_plan_trace.py makes them): seeded N(0, 1) maps of 16 x 16 (feat) and 32 x 32 (tmpx) texels, rounded to the
storage type (the sort cases: one image of 128 x 128); head weights N(0, 1) * fan_in ** -0.5 and biases N(0, 0.01); synth_points;
N(0, 1) upstream gradients of the live heads; the surface step with k = 0 and k = 1, thr the reference's median in-image df[:, k].

Bounds: the project's own (tests/test_gpu_query.py, tests/test_gpu_wgrad_kernels.py), measured against query_ref in float64:
  outputs (df, pca, parts, centers, X, H)               5e-5 * max(1, max |ref|)
  gradients (dpoints, dX, dZ, the step's displacement)  2e-5 * max |ref| of that tensor
Where query_ref's own formulas evaluated in float32 miss a bound, no float32 kernel can be held to it: the bound of that quantity
at that case is four times that float32 error (a kernel's summation order differs): FLOORS, the measured figure next to the case."""
import zlib

import numpy as np

import query_plan_cases as qc
from query_plan_cases import BF16, BWD_POINTS, BWD_TRAIN, F16, F16X3, F32, FWD, FWD_TRAIN, HF, SURFACE_STEP, WS, X3

OUT_BOUND, GRAD_BOUND = 5e-5, 2e-5
# the exclusions, conditions on the reference alone.  The ReLU margin is query_ref's: the smaller of its float64 evaluations at the
# exact sample coordinates and at the float32-rounded ones -- on these maps the rounding of a coordinate moves X, and with it a
# pre-activation, by more than 5e-6, and a kernel's ReLU decides on the float32 X (which it is held to bit for bit)
MARGIN_MIN, LINE_MIN, BORDER_MIN, CLAMP_MIN = 5e-6, 1e-5, 1e-6, 1e-5
MAX_EXCLUDED = 0.05
MAX_POINTS = 4 * 6200
TH = TW = 32
OP_NAMES = {FWD: "fwd", FWD_TRAIN: "fwd_train", BWD_POINTS: "bwd_points", SURFACE_STEP: "surface_step", BWD_TRAIN: "bwd_train"}
DT_NAMES = {F32: "f32", BF16: "bf16", F32 | X3: "f32+x3", BF16 | X3: "bf16+x3", F16X3: "f16x3", F16: "f16", F16 | X3: "f16+x3"}

_W8T = ('query_fwd_f32_w8_kernel<float, true, false>', 'query_fwd_f32_kernel<float, 2, true, false>',
        'query_fwd_f32_w8_kernel<float, true, false>', 'query_fwd_f32_w8_kernel<float, true, false>')
_BW4 = 'query_bwd_f32_kernel<float, false, 1, false, 4, false, false, false>'
_BX4 = 'query_bwd_f32_kernel<float, false, 1, false, 4, true, false, false>'
_SURF = 'query_bwd_f32_kernel<float, false, 1, false, 4, true, true, false>'
# rows the plan file does not have, in its format
EXTRA = [
    (FWD_TRAIN, F32, 1, 1, 16, 16, 0, 0, _W8T),
    (FWD_TRAIN, F32, 1, 63, 16, 16, 0, 0, _W8T),
    (BWD_TRAIN, F32, 1, 1, 16, 16, 15, HF, 'query_bwd_f32_kernel<float, true, 2, true, 4, false, false, false>'),
    (BWD_TRAIN, F32, 1, 63, 16, 16, 15, HF, 'query_bwd_f32_kernel<float, true, 2, true, 4, false, false, false>'),
    (BWD_TRAIN, F32, 1, 1, 16, 16, 15, 0, 'query_bwd_f32_kernel<float, true, 2, false, 4, false, false, false>'),
    (BWD_TRAIN, F32, 1, 63, 16, 16, 15, 0, 'query_bwd_f32_kernel<float, true, 2, false, 4, false, false, false>'),
    (SURFACE_STEP, F16X3, 1, 1, 16, 16, 0, 0, _SURF),
    (SURFACE_STEP, F16X3, 1, 63, 16, 16, 0, 0, _SURF),
    (BWD_POINTS, F32, 2, 333, 16, 16, 5, 0, _BW4),              # parts and centers absent
    (BWD_POINTS, F16X3, 2, 333, 16, 16, 10, 0, _BX4),           # df and pca absent
]
# rows of the plan file that run under every set besides the selected ones
ALWAYS = ([c for c in qc.CASES if c[3] in (1, 63, 65)] +
          [c for c in qc.CASES if c[:6] == (BWD_POINTS, F16X3, 4, 4097, 16, 16) and c[6] in (1, 2, 4, 8)] +
          [c for c in qc.CASES if c[:7] == (BWD_POINTS, F16X3, 4, 4160, 16, 16, 15)])

# Where float32 itself misses a bound: (case id, quantity) -> (the float32 error of query_ref's formulas against float64, the bound
# = 4 x that), both in the units of the bound they replace (a multiple of max |ref|).  `python tests/query_kernel_cases.py` prints
# these rows.  The step's displacement divides by the gradient's norm: among 16 000 points some gradients are small enough for
# the float32 rounding of the sample coordinates to turn them; the one-point training backward has only its own gradient as scale.
FLOORS = {
    ("bwd_train-f32-1x1-16x16-l15-f2", "dpoints"): (2.09e-05, 8.36e-05),
    ("surface_step-f16x3-4x4097-16x16-l0-f0", "step0"): (3.53e-05, 1.41e-04),
    ("surface_step-f16x3-4x6200-16x16-l0-f0", "step0"): (7.32e-05, 2.93e-04),
    ("surface_step-f16x3-4x6200-16x16-l0-f0", "step1"): (3.94e-05, 1.58e-04),
    ("surface_step-bf16+x3-4x4097-16x16-l0-f0", "step0"): (3.71e-05, 1.48e-04),
    ("surface_step-bf16+x3-4x6200-16x16-l0-f0", "step0"): (7.25e-05, 2.90e-04),
    ("surface_step-bf16+x3-4x6200-16x16-l0-f0", "step1"): (3.97e-05, 1.59e-04),
    ("surface_step-f16-4x4097-16x16-l0-f0", "step0"): (3.48e-05, 1.39e-04),
    ("surface_step-f16-4x6200-16x16-l0-f0", "step0"): (7.62e-05, 3.05e-04),
    ("surface_step-f16-4x6200-16x16-l0-f0", "step1"): (3.79e-05, 1.51e-04),
}


def case_id(c):
    return "%s-%s-%dx%d-%dx%d-l%d-f%d" % (OP_NAMES[c[0]], DT_NAMES[c[1]], c[2], c[3], c[4], c[5], c[6], c[7])


def map_type(dtype):
    return F32 if dtype == F16X3 else dtype & ~X3


def _size(c):
    return (c[2] * c[3], c[4] * c[5])


def selected(k):
    """the cases of switch set k, in the order they run"""
    pool = [c for c in qc.CASES if c[3] != 20000]
    best = {}
    for c in pool:
        key = qc.expected(c, k)
        if key not in best or _size(c) < _size(best[key]):
            best[key] = c
    out = list(best.values())
    for c in ALWAYS + EXTRA:
        if c not in out:
            out.append(c)
    # the forward a staged backward reads
    for c in list(out):
        if c[0] == BWD_TRAIN and c[7] & HF:
            fwd = [d for d in qc.CASES + EXTRA if d[0] == FWD_TRAIN and d[1:6] == c[1:6]]
            assert fwd, c
            if fwd[0] not in out:
                out.append(fwd[0])
    assert all(c[2] * c[3] <= MAX_POINTS for c in out)
    return sorted(out, key=lambda c: (map_type(c[1]), c[4], c[5], c[2], c[3], c[0], c[1], c[6], c[7]))


def jobs_of(k):
    """[(case, kernel name, sort)] of switch set k"""
    return [(c,) + qc.expected(c, k) for c in selected(k)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def round_to(a, mt):
    """float32 array -> the float32 values its storage type holds"""
    if mt == BF16:
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()
    return a.astype(np.float16).astype(np.float32) if mt == F16 else a


_MAPS = {}


def maps_of(mt, FH, FW):
    """(feat (Bm, FH, FW, 256), tmpx (Bm, 32, 32, 64)) float32 NHWC, as stored: four images, one for the large maps of the sort cases"""
    if (mt, FH, FW) not in _MAPS:
        Bm = 4 if FH * FW <= 1024 else 1
        r = _rng("maps", FH, FW)
        _MAPS[mt, FH, FW] = (round_to(r.standard_normal((Bm, FH, FW, 256), dtype=np.float32), mt),
                             round_to(r.standard_normal((Bm, TH, TW, 64), dtype=np.float32), mt))
    return _MAPS[mt, FH, FW]


_WEIGHTS = {}


def weights():
    """state dict of the four heads, float32 (out, in)"""
    if not _WEIGHTS:
        r = _rng("heads")
        for hd, odim in (("df", 2), ("part_predictor", 14), ("pca_predictor", 9), ("center_predictor", 6)):
            for l, (i, o) in enumerate(((323, 128), (128, 128), (128, 128), (128, odim))):
                _WEIGHTS["%s.%d.weight" % (hd, 2 * l)] = (r.standard_normal((o, i), dtype=np.float32) * np.float32(i ** -0.5)).astype(np.float32)
                _WEIGHTS["%s.%d.bias" % (hd, 2 * l)] = (r.standard_normal(o, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    return _WEIGHTS


POINT_SEED = {}          # (B, N) -> seed of synth_points where the default leaves no point outside the image
CROP_CENTER = (1008.0, 995.0)


def points_of(B, N):
    from chore_amd.utils import synth
    assert synth.CROP_CENTER == CROP_CENTER
    return synth.synth_points(B, N, seed=POINT_SEED.get((B, N), 3)), np.tile(np.array([CROP_CENTER], np.float32), (B, 1))


def grads_of(c):
    """upstream gradients of df, parts, pca, centers (the heads' order; bit h of the live mask), None where absent"""
    r = _rng("grads", case_id(c))
    return [r.standard_normal((c[2], odim, c[3]), dtype=np.float32) if c[6] >> h & 1 else None for h, odim in enumerate((2, 14, 9, 6))]


def surface_thr(f, k):
    """the threshold of a surface step: the reference's median in-image df[:, k] (float32), so that both sides of the clamp occur"""
    inside = f["in_img"]
    return float(np.float32(np.median(f["df"][:, k][inside]))) if inside.any() else 0.3


# ---------------------------------------------------------------------------------------------------------------- coverage
_TX = (("float", False), ("unsigned short", False), ("float", True), ("unsigned short", True), ("qh16_t", True))     # launch_query_*_t<T, X3>


def _b(v):
    return "true" if v else "false"


def instantiations():
    """the 56 instantiations launch_query_fwd and launch_query_bwd spell out, as rocprofv3 names them: pattern (the spelling in the
    source, T and X3 open) -> names"""
    t = {}
    for T, x3 in _TX:
        h16 = T == "qh16_t"

        def add(pattern, name):
            t.setdefault(pattern, []).append(name)
        if x3:
            for ncb in (1, 2):
                add("query_fwd_x3_split_kernel<T, %d>" % ncb, "query_fwd_x3_split_kernel<%s, %d>" % (T, ncb))
        if not h16:
            add("query_fwd_f32_w8_kernel<T, true, X3>", "query_fwd_f32_w8_kernel<%s, true, %s>" % (T, _b(x3)))
            add("query_fwd_f32_kernel<T, 2, true, X3>", "query_fwd_f32_kernel<%s, 2, true, %s>" % (T, _b(x3)))
        if not x3:
            add("query_fwd_f32_w8_kernel<T, false, false>", "query_fwd_f32_w8_kernel<%s, false, false>" % T)
        for ncb in (1, 2):
            add("query_fwd_f32_kernel<T, %d, false, X3>" % ncb, "query_fwd_f32_kernel<%s, %d, false, %s>" % (T, ncb, _b(x3)))
        bw = lambda *a: "query_bwd_f32_kernel<%s, %s>" % (T, ", ".join(_b(v) if isinstance(v, bool) else str(v) for v in a))  # noqa: E731
        if x3 and not h16:
            add("launch_k<T, true, 1, true, 8, true>", bw(True, 1, True, 8, True, False, False))
        if not x3:
            add("launch_k<T, true, 2, true, 4, false>", bw(True, 2, True, 4, False, False, False))
            add("launch_k<T, true, 2, false, 4, false>", bw(True, 2, False, 4, False, False, False))
            add("launch_k<T, false, 1, false, 8, false>", bw(False, 1, False, 8, False, False, False))
        if x3:
            add("launch_k<T, false, 2, false, 4, true, true, true>", bw(False, 2, False, 4, True, True, True))
            add("launch_k<T, false, 2, false, 4, true, false, true>", bw(False, 2, False, 4, True, False, True))
            add("launch_k<T, false, 1, false, 4, true, true>", bw(False, 1, False, 4, True, True, False))
            add("launch_k<T, false, 2, false, 4, true, true>", bw(False, 2, False, 4, True, True, False))
        for ncb in (1, 2):
            add("launch_k<T, false, %d, false, 4, X3>" % ncb, bw(False, ncb, False, 4, x3, False, False))
    return t


# instantiations no case reaches: name -> the reason
NOT_REACHED = {
}


# ---------------------------------------------------------------------------------------------------------------- the float32 floor
def exclusions(f):
    """(rows compared for outputs, rows compared for gradients) of a reference forward"""
    ok_out = ~((f["margin"] < MARGIN_MIN) | (f["border"] < BORDER_MIN))
    return ok_out, ok_out & ~(f["line"] < LINE_MIN)


def floors_of(c, f, f32):
    """quantity -> (the error of query_ref in float32 (f32) against float64 (f), in the units of the quantity's bound; that bound)
    for every quantity the GPU test compares at case c"""
    import query_ref as qr
    P = c[2] * c[3]
    ok_out, ok_grad = exclusions(f)

    def err(a, b, ok, floor_one):
        a, b = np.asarray(a, np.float64).reshape(P, -1), np.asarray(b).reshape(P, -1)
        scale = max(1.0, np.abs(b).max()) if floor_one else np.abs(b).max()
        return float(np.abs(a - b)[ok].max() / scale) if ok.any() and scale > 0 else 0.0

    def rows(a):
        return a.reshape(c[2], -1, c[3]).transpose(0, 2, 1)
    out = {}
    if c[0] in (FWD, FWD_TRAIN):
        for q in qr.OUT_NAMES:
            out[q] = (err(rows(f32[q]), rows(f[q]), ok_out, True), OUT_BOUND)
    if c[0] in (FWD_TRAIN, BWD_TRAIN):
        out["X"] = (err(f32["X"], f["X"], ok_out, True), OUT_BOUND)
        st = lambda H: np.stack([np.stack(r) for r in H]).transpose(2, 0, 1, 3)  # noqa: E731
        out["H"] = (err(st(f32["H"]), st(f["H"]), ok_out, True), OUT_BOUND)
    if c[0] in (BWD_POINTS, BWD_TRAIN):
        g = grads_of(c)
        b, b32 = qr.backward(f, g), qr.backward(f32, g)
        out["dpoints"] = (err(b32["dpoints"], b["dpoints"], ok_grad, False), GRAD_BOUND)
        if c[0] == BWD_TRAIN:
            out["dX"] = (err(b32["dX"], b["dX"], ok_grad, False), GRAD_BOUND)
            out["dZ"] = (err(st(b32["dZ"]), st(b["dZ"]), ok_grad, False), GRAD_BOUND)
    if c[0] == SURFACE_STEP:
        for k in (0, 1):
            thr = surface_thr(f, k)
            (o, clamp), (o32, _) = qr.surface_step(f, k, thr), qr.surface_step(f32, k, thr)
            out["step%d" % k] = (err(o32.astype(np.float64) - f["points"], o - f["points"], ok_grad & ~(clamp < CLAMP_MIN), False), GRAD_BOUND)
    return out


def forwards_of(c, both=False):
    """the reference forward of a case in float64, and in float32 if asked for"""
    import query_ref as qr
    feat, tmpx = maps_of(map_type(c[1]), c[4], c[5])
    pts, cc = points_of(c[2], c[3])
    a = (pts, cc, feat[:c[2]], tmpx[:c[2]], weights())
    return (qr.forward(*a), qr.forward(*a, np.float32)) if both else qr.forward(*a)


if __name__ == "__main__":       # prints the rows of FLOORS: every (case, quantity) whose float32 error exceeds its bound
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    seen = {}
    for k_ in range(len(qc.SWITCH_SETS)):
        for c_ in selected(k_):
            seen.setdefault((map_type(c_[1]), c_[4], c_[5], c_[2], c_[3]), {})[case_id(c_)] = c_
    for key_, cs_ in sorted(seen.items()):
        f_, f32_ = forwards_of(next(iter(cs_.values())), True)
        for cid_, c_ in cs_.items():
            for q_, (e_, b_) in floors_of(c_, f_, f32_).items():
                if e_ > b_:
                    print('    ("%s", "%s"): (%.2e, %.2e),' % (cid_, q_, e_, 4 * e_))
