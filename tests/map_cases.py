"""The case matrix, the inputs and the coverage table of tests/test_gpu_map_kernels.py (no GPU needed to import this).

The encoder's map operators: csrc/enc_misc.hip behind the entry points of csrc/ops.hip -- GroupNorm statistics and apply, 2x2
average pooling, bicubic x2 upsampling + add and its transpose, the two 7x7 stems, max |x|.  A case is a dict with an `id`; CASES
maps a family (one GPU test each) to its cases.  The shapes were chosen by reading the kernels, around the constants below: one
tile, one tile and a ragged rest in each direction, a slice count at its clamp, a grid at its cap, the boundary between the
unrolled part and the tail of a loop.  COVERAGE has one row per entry point: the ids of the cases that call it, or the reason
none needs to.  tests/test_map_coverage_table.py holds the table against _lib.py, the constants against the sources and the case
families against the GPU test module.

Kinds.  "random": standard normal values.  "exact": integers in {-2 ... 2}, arranged per family so that every output and every sum
is exactly representable -- then the result must come out bit for bit, and one dropped or doubled value shows:
  gn_stats, pool, pool_bwd, absmax  integers in, integers or quarters out
  stem, stem_x3                     integer images, weights in {-1, 0, 1} with at most 12 taps per output channel, integer bias
  upadd                             the weights of the interpolation, taken at multiples of (n - 1) / (2 n - 1), are no dyadic
                                    rationals, so an interpolated value is never exact: `low` is zero (a + 0: values and statistics
                                    exact, every pixel of `a` must arrive once) except at H = W = 1, where the weights are 0 and 1
  up2_bwd                           dy is zero but for pixel (0, 0) of every image, whose weights are exactly 1 on (0, 0) and 0
                                    elsewhere: the result is that pixel at (0, 0) and an exact zero everywhere else
  gn_relu                           gamma = 0 and an integer beta: y = relu(beta) whatever the statistics say"""
import zlib

import numpy as np

# ---- the constants the shapes were chosen around (held equal to the sources by test_map_coverage_table.py) ----
CONSTANTS = {
    "MAP_T": 8,                  # enc_misc.hip: output rows of a map_stats_kernel tile (and the columns of a PoolOp tile)
    "UP_CT": 64,                 # UpAddOp::CT: channels of a workgroup
    "UP_TW": 16,                 # UpAddOp::TW: output columns of a tile
    "UP_PS": 8,                  # UpAddOp::PS: staged source rows
    "UP_PSX": 12,                # UpAddOp::PSX = TW / 2 + 4: staged source columns
    "STEM_T": 16,                # stem_kernel: tile edge (stem_x3_kernel: tile rows)
    "STEM_MAXC": 8,              # stem_kernel: most input channels
    "SX_TW": 32,                 # stem_x3_kernel: tile columns
    "AMAX_CELLS": 256,           # enc_common.h: workgroups (and cells) of absmax_f32_kernel
    "GN_SLICE_PIXELS": 64,       # gn_splits: at least this many pixels per slice ...
    "GN_SLICES_MAX": 256,        # ... and at most this many slices per image
    "GN_APPLY_BLOCKS": 1024,     # launch_gn_apply_relu: cap of the grid (256 with statistics)
    "GN_APPLY_BLOCKS_STATS": 256,
    "UP2_NC": 12,                # up2_bwd_kernel: candidate rows / columns of a low-resolution pixel, from max(0, 2 l - 5)
}
F32, BF16, F16 = "f32", "bf16", "f16"
DTYPES = (F32, BF16, F16)
KINDS = ("random", "exact")
UNKNOWN_DTYPE = 7                # no CHORE_* element type
EXACT_STEM_TAPS = 12             # non-zero taps per output channel of an exact-kind stem: |y| <= 12 * 2 + 2, exact in bf16


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


CASES = {}


def _add(family, name, **kw):
    CASES.setdefault(family, []).append(dict(kw, id="%s.%s" % (family, name), family=family))


def ids(family):
    return [c["id"] for c in CASES[family]]


def values(c, shape, *key):
    """float32 values of the case's kind"""
    r = rng(c["id"], *key)
    if c["kind"] == "exact":
        return r.integers(-2, 3, shape).astype(np.float32)
    return r.standard_normal(shape, dtype=np.float32)


# ================================================================================================ chore_gn_stats
# HW = 1, 63: one slice; 64: one slice of exactly 64 pixels; 129: two slices of 64 and 65; 64 * 256 + 1: the slice count clamps at 256.
# Every case runs twice: zeroed = 0 on accumulators full of garbage, zeroed = 1 on zeros.
GN_C = (32, 64, 128, 256)
GN_STATS_HW = (1, 63, 64, 129, 64 * 256 + 1)
for _kind in KINDS:
    for _C in GN_C:
        for _HW in GN_STATS_HW:
            _add("gn_stats", "C%d.HW%d.B3.f32.%s" % (_C, _HW, _kind), C=_C, HW=_HW, B=3, dtype=F32, kind=_kind)
    _add("gn_stats", "C64.HW129.B1.f32.%s" % _kind, C=64, HW=129, B=1, dtype=F32, kind=_kind)
    for _dt in (BF16, F16):
        for _C, _HW, _B in ((64, 129, 3), (256, 63, 1), (32, 64 * 256 + 1, 1), (128, 1, 3)):
            _add("gn_stats", "C%d.HW%d.B%d.%s.%s" % (_C, _HW, _B, _dt, _kind), C=_C, HW=_HW, B=_B, dtype=_dt, kind=_kind)


def gn_stats_chain(C, HW):
    """(L, P, adds): the longest per-thread chain, the partials a channel's reducer adds, the atomic adds per cell"""
    S = min(max(HW // CONSTANTS["GN_SLICE_PIXELS"], 1), CONSTANTS["GN_SLICES_MAX"])
    P = 256 // (C // 4)
    longest = max((HW * (s + 1)) // S - (HW * s) // S for s in range(S))
    return -(-longest // P), P, S


# ================================================================================================ chore_gn_relu_fwd
# HW = 4097 with C = 256: 4097 * 64 vectors are more than 1024 workgroups of 256 hold -- the grid-stride loop runs twice.
# HW = 1 goes with C = 128 and 256 only: a group of one value (C = 32) or two (C = 64) has a variance of zero or of any size, the
# result is what is left of x * rstd - mean * rstd with rstd up to 316 -- the cancellation of any fp32 evaluation, not the kernel's.
# stats "ref": the float64 statistics of the stored input, encoded into the cells by map_ref.stats_encode; "device": chore_gn_stats
GN_RELU_HW = (1, 100, 4097)
for _C in GN_C:
    for _dt in DTYPES:
        for _HW in GN_RELU_HW:
            if _HW == 1 and _C < 128:
                continue
            _add("gn_relu", "C%d.HW%d.%s.random" % (_C, _HW, _dt), C=_C, HW=_HW, B=3 if _HW == 100 else 1, dtype=_dt, kind="random", stats="ref")
        _add("gn_relu", "C%d.HW100.%s.exact" % (_C, _dt), C=_C, HW=100, B=3, dtype=_dt, kind="exact", stats="ref")
for _dt in DTYPES:
    _add("gn_relu", "C128.HW100.%s.device_stats" % _dt, C=128, HW=100, B=3, dtype=_dt, kind="random", stats="device")


# ================================================================================================ chore_avgpool2_fwd / _bwd
# input (H, W): (2, 2) one output pixel; (16, 16) exactly one 8 x 8 output tile; (18, 14) ragged both ways (9 x 7 outputs: two tiles
# down, a short one across); (2, 34) 1 x 17 outputs: three tiles across.  Every forward case runs with and without out_stats.
POOL_HW = ((2, 2), (16, 16), (18, 14), (2, 34))
for _kind in KINDS:
    for _C in (64, 128, 256):
        for _H, _W in POOL_HW:
            for _B in (1, 3):
                for _dt in (F32, BF16):
                    _add("pool", "C%d.%dx%d.B%d.%s.%s" % (_C, _H, _W, _B, _dt, _kind), C=_C, H=_H, W=_W, B=_B, dtype=_dt, kind=_kind)
    for _C in (4, 36, 64, 128, 256):
        for _i, (_H, _W) in enumerate(POOL_HW):
            for _dt in (F32, BF16):
                _B = 3 if (_i + _C // 4) % 2 else 1
                _add("pool_bwd", "C%d.%dx%d.B%d.%s.%s" % (_C, _H, _W, _B, _dt, _kind), C=_C, H=_H, W=_W, B=_B, dtype=_dt, kind=_kind)


def map_chain(C, CT, TW):
    """(L, P) of map_stats_kernel: a thread stores ceil(TW / P) columns of MAP_T rows; the reducer adds P partials"""
    P = 256 // (CT // 4)
    return -(-TW // P) * CONSTANTS["MAP_T"], P


# ================================================================================================ chore_upadd_fwd
# low-resolution (H, W): the output of (4, 8) is exactly one 8 x 16 tile; (5, 9) is ragged in both directions, (4, 9) in x only;
# (128, 3), (3, 128), (255, 2): a long axis (the source coordinate is an fp32 product of up to 509 * 254 / 509).
UPADD_HW = ((1, 1), (2, 2), (2, 3), (4, 8), (5, 9), (4, 9), (12, 17), (128, 3), (3, 128), (255, 2))
UPADD_LARGE = ((128, 3), (3, 128), (255, 2))
for _kind in KINDS:
    for _i, (_H, _W) in enumerate(UPADD_HW):
        _B = 1 if (_H, _W) in UPADD_LARGE or _i % 2 else 3
        _add("upadd", "C64.%dx%d.B%d.f32.%s" % (_H, _W, _B, _kind), C=64, H=_H, W=_W, B=_B, dtype=F32, kind=_kind, inplace=False)
    for _C in (64, 128, 256):
        for _j, _dt in enumerate(DTYPES):
            if (_C, _dt) != (64, F32):
                _B = 3 if (_C // 64 + _j) % 2 else 1
                _add("upadd", "C%d.5x9.B%d.%s.%s" % (_C, _B, _dt, _kind), C=_C, H=5, W=9, B=_B, dtype=_dt, kind=_kind, inplace=False)
    for _dt in DTYPES:
        _add("upadd", "C64.5x9.B3.%s.%s.inplace" % (_dt, _kind), C=64, H=5, W=9, B=3, dtype=_dt, kind=_kind, inplace=True)
ADJOINT_HW = ((2, 3), (5, 9), (12, 17))


def gn_relu_affine(c):
    """-> gamma, beta (C) float32; exact kind: gamma = 0, an integer beta"""
    r = rng(c["id"], "affine")
    if c["kind"] == "exact":
        return np.zeros(c["C"], np.float32), r.integers(-2, 3, c["C"]).astype(np.float32)
    return r.random(c["C"], dtype=np.float32) + np.float32(0.5), r.standard_normal(c["C"], dtype=np.float32) * np.float32(0.2)


def upadd_inputs(c):
    """-> a (B,2H,2W,C), low (B,H,W,C) float32; exact kind: low = 0 unless H = W = 1"""
    a = values(c, (c["B"], 2 * c["H"], 2 * c["W"], c["C"]), "a")
    low = values(c, (c["B"], c["H"], c["W"], c["C"]), "low")
    if c["kind"] == "exact" and (c["H"], c["W"]) != (1, 1):
        low[:] = 0.0
    return a, low


def up2_bwd_input(c):
    """-> dy (B,2H,2W,C) float32; exact kind: zero but for pixel (0, 0) of every image"""
    dy = values(c, (c["B"], 2 * c["H"], 2 * c["W"], c["C"]))
    if c["kind"] == "exact":
        keep = dy[:, 0, 0].copy()
        dy[:] = 0.0
        dy[:, 0, 0] = keep
    return dy


# ================================================================================================ chore_up2_bwd
# every n from 2 to 20 on one axis (the 12-candidate window from max(0, 2 l - 5) must hold every high-resolution coordinate that
# weighs on l: at the low edge, in the middle, at the high edge), the other axis 2, 3 or 7; then the long axes.
UP2_OTHER = (2, 3, 7)
UP2_SIZES = [(n, UP2_OTHER[(n - 2) % 3]) for n in range(2, 21)] + [(UP2_OTHER[(n - 2) % 3], n) for n in range(2, 21)] + [(128, 3), (3, 128), (255, 2)]
UP2_WIDE_SIZES = ((5, 3), (12, 7), (3, 128))
for _kind in KINDS:
    for _i, (_H, _W) in enumerate(UP2_SIZES):
        _add("up2_bwd", "C4.%dx%d.B%d.f32.%s" % (_H, _W, 1 + 2 * (_i % 2), _kind), C=4, H=_H, W=_W, B=1 + 2 * (_i % 2), dtype=F32, kind=_kind)
    for _H, _W in (UP2_SIZES[0], UP2_SIZES[3], UP2_SIZES[10], UP2_SIZES[18], (255, 2)):
        _add("up2_bwd", "C4.%dx%d.B3.bf16.%s" % (_H, _W, _kind), C=4, H=_H, W=_W, B=3, dtype=BF16, kind=_kind)
    for _C in (64, 256):
        for _i, (_H, _W) in enumerate(UP2_WIDE_SIZES):
            for _dt in (F32, BF16):
                _B = 3 if _i == 1 else 1
                _add("up2_bwd", "C%d.%dx%d.B%d.%s.%s" % (_C, _H, _W, _B, _dt, _kind), C=_C, H=_H, W=_W, B=_B, dtype=_dt, kind=_kind)


# ================================================================================================ chore_stem_fwd / chore_stem_x3_fwd
# image (H, W): (2, 2) one output pixel; (32, 32) exactly one 16 x 16 tile; (34, 30) 17 x 15: ragged both ways; (22, 18) the size of
# test_gpu_train_ops.py; (64, 66) 32 x 33 outputs: a second SX_TW column block of one column.  The x3 cases run with and without
# out_stats.
STEM_HW = ((2, 2), (32, 32), (34, 30), (22, 18))
STEM_X3_HW = STEM_HW + ((64, 66),)
for _kind in KINDS:
    for _Cin in (1, 3, 4, 5, 8):
        for _i, (_H, _W) in enumerate(STEM_HW):
            _B = 1 + (_i + _Cin) % 2
            _add("stem", "Cin%d.%dx%d.B%d.f32.%s" % (_Cin, _H, _W, _B, _kind), Cin=_Cin, H=_H, W=_W, B=_B, dtype=F32, kind=_kind)
        _add("stem", "Cin%d.34x30.B2.bf16.%s" % (_Cin, _kind), Cin=_Cin, H=34, W=30, B=2, dtype=BF16, kind=_kind)
    for _H, _W in ((2, 2), (32, 32), (22, 18)):
        _add("stem", "Cin5.%dx%d.B1.bf16.%s" % (_H, _W, _kind), Cin=5, H=_H, W=_W, B=1, dtype=BF16, kind=_kind)
    for _Cin in (3, 4, 5):
        for _i, (_H, _W) in enumerate(STEM_X3_HW):
            _B = 1 + (_i + _Cin) % 2
            _add("stem_x3", "Cin%d.%dx%d.B%d.%s" % (_Cin, _H, _W, _B, _kind), Cin=_Cin, H=_H, W=_W, B=_B, dtype=F32, kind=_kind)
STEM_X3_CHAIN = (8, 32 + 4)      # L: a lane's four pixels x two channels of a group; P: the 32 lanes of a half wave and the four waves


def stem_inputs(c):
    """-> images (B,Cin,H,W), w (64,Cin,7,7), bias (64) float32"""
    B, Cin, H, W = c["B"], c["Cin"], c["H"], c["W"]
    img = values(c, (B, Cin, H, W), "img")
    if c["kind"] == "exact":
        r = rng(c["id"], "w")
        w = np.zeros((64, Cin * 49), np.float32)
        for o in range(64):
            w[o, r.choice(Cin * 49, EXACT_STEM_TAPS, replace=False)] = r.choice(np.float32([-1.0, 1.0]), EXACT_STEM_TAPS)
        return img, w.reshape(64, Cin, 7, 7), r.integers(-2, 3, 64).astype(np.float32)
    return img, values(c, (64, Cin, 7, 7), "w") * np.float32(0.1), values(c, (64,), "bias")


# ================================================================================================ chore_absmax_f32
# a thread holds eight 16-byte loads in flight, AMAX_CELLS * 256 vectors apart: U floats make one unrolled step of the whole grid
ABSMAX_STRIDE = CONSTANTS["AMAX_CELLS"] * 256                # vectors between two loads of a thread
ABSMAX_U = 8 * ABSMAX_STRIDE * 4
ABSMAX_N = (4, 1024, ABSMAX_U - 4, ABSMAX_U, ABSMAX_U + 4, 2 * ABSMAX_U + 1028)
ABSMAX_PLACES = ("first", "last", "last_unrolled", "first_tail")


def absmax_place(n, place):
    """the vector that holds the maximum, or None where the loop has no such part: restates which vectors the unrolled loop
    (i + 7 stride < n4, steps of 8 stride) and the tail loop of a thread read"""
    n4, s = n // 4, ABSMAX_STRIDE
    if place == "first":
        return 0
    if place == "last":
        return n4 - 1
    t = np.arange(min(s, n4), dtype=np.int64)
    steps = np.maximum(0, -(-(n4 - 7 * s - t) // (8 * s)))       # unrolled steps of thread t
    if place == "last_unrolled":
        return int((t + steps * 8 * s - s)[steps > 0].max()) if (steps > 0).any() else None
    tail = t + steps * 8 * s                                     # the first vector a thread's tail loop reads
    return int(tail[tail < n4].min()) if (tail < n4).any() else None


_i = 0
for _kind in KINDS:
    for _n in ABSMAX_N:
        _seen = set()
        for _place in ABSMAX_PLACES:
            _v = absmax_place(_n, _place)
            if _v is None or _v in _seen:
                continue
            _seen.add(_v)
            _add("absmax", "n%d.%s.%s.%s" % (_n, _place, "neg" if _i % 2 else "pos", _kind), n=_n, place=_place, vec=_v, neg=bool(_i % 2),
                 kind=_kind, special=None)
            _i += 1
for _special in ("denormal", "inf", "zero"):
    _add("absmax", "n%d.%s" % (ABSMAX_U + 4, _special), n=ABSMAX_U + 4, place="first_tail", vec=absmax_place(ABSMAX_U + 4, "first_tail"), neg=False,
         kind="exact", special=_special)


def absmax_input(c):
    """-> x (n) float32 whose largest magnitude sits in one element of vector c["vec"]"""
    n, v = c["n"], c["vec"]
    at = 4 * v + v % 4
    if c["special"]:
        x = np.zeros(n, np.float32)
        if c["special"] == "denormal":       # every non-zero value a denormal: the maximum is one too
            x[::7] = np.float32(1e-42)
            x[at] = np.float32(3e-41)
        elif c["special"] == "inf":
            x[::5] = np.float32(1.5)
            x[at] = np.float32(np.inf)
        return x
    x = values(c, (n,), "x")
    x[at] = 0.0
    x[at] = (np.abs(x).max() + np.float32(1.0)) * np.float32(-1.0 if c["neg"] else 1.0)
    return x


# ================================================================================================ refusals
# rc = -1 with a message of the entry point, before any launch: guarded outputs and statistics untouched.  `over` replaces
# arguments of a small valid call of the entry point (tests/test_gpu_map_kernels.py: _REFUSED_BASE); `msg` must be in the message
def _refuse(fn, name, msg, **over):
    _add("refused", "%s.%s" % (fn.replace("chore_", ""), name), fn=fn, over=over, msg=msg)


for _C in (0, 16, 288):
    _refuse("chore_gn_stats", "C%d" % _C, "unsupported C=%d" % _C, C=_C)
for _C in (96, 160, 192, 224):           # C / 32 no power of two: group_lane_sum's xor tree would mix neighbouring groups
    _refuse("chore_gn_stats", "C%d" % _C, "unsupported C=%d" % _C, C=_C)
_refuse("chore_gn_stats", "B0", "chore_gn_stats", B=0)
_refuse("chore_gn_stats", "Bneg", "chore_gn_stats", B=-1)
_refuse("chore_gn_stats", "HW0", "chore_gn_stats", HW=0)
_refuse("chore_gn_stats", "HWneg", "chore_gn_stats", HW=-5)
_refuse("chore_gn_stats", "dtype", "chore_gn_stats", dtype=UNKNOWN_DTYPE)
for _C in (0, -32, 288, 96):
    _refuse("chore_gn_relu_fwd", "C%d" % _C, "unsupported C=%d" % _C, C=_C)
_refuse("chore_gn_relu_fwd", "B0", "chore_gn_relu_fwd", B=0)
_refuse("chore_gn_relu_fwd", "Bneg", "chore_gn_relu_fwd", B=-2)
_refuse("chore_gn_relu_fwd", "HW0", "chore_gn_relu_fwd", HW=0)
_refuse("chore_gn_relu_fwd", "HWneg", "chore_gn_relu_fwd", HW=-1)
_refuse("chore_gn_relu_fwd", "dtype", "chore_gn_relu_fwd", dtype=UNKNOWN_DTYPE)
_refuse("chore_avgpool2_fwd", "C32", "unsupported C=32", C=32)
_refuse("chore_avgpool2_fwd", "odd_H", "chore_avgpool2_fwd", H=5)
_refuse("chore_avgpool2_fwd", "f16", "chore_avgpool2_fwd", dtype=F16)
_refuse("chore_avgpool2_bwd", "f16", "chore_avgpool2_bwd", dtype=F16)
_refuse("chore_upadd_fwd", "C32", "unsupported C=32", C=32)
for _k in ("B", "H", "W"):
    _refuse("chore_upadd_fwd", "%s0" % _k, "chore_upadd_fwd", **{_k: 0})
    _refuse("chore_upadd_fwd", "%sneg" % _k, "chore_upadd_fwd", **{_k: -3})
_refuse("chore_upadd_fwd", "dtype", "chore_upadd_fwd", dtype=UNKNOWN_DTYPE)
_refuse("chore_up2_bwd", "H1", "up2_bwd", H=1)
_refuse("chore_up2_bwd", "C6", "up2_bwd", C=6)
_refuse("chore_up2_bwd", "C0", "up2_bwd", C=0)
_refuse("chore_up2_bwd", "B0", "up2_bwd", B=0)
_refuse("chore_up2_bwd", "Bneg", "up2_bwd", B=-1)
_refuse("chore_up2_bwd", "f16", "chore_up2_bwd", dtype=F16)
_refuse("chore_up2_bwd", "dtype", "chore_up2_bwd", dtype=UNKNOWN_DTYPE)
_refuse("chore_stem_fwd", "Cin9", "Cin > 8", Cin=CONSTANTS["STEM_MAXC"] + 1)
_refuse("chore_stem_fwd", "odd_W", "chore_stem_fwd", W=7)
_refuse("chore_stem_fwd", "f16", "chore_stem_fwd", dtype=F16)
_refuse("chore_stem_x3_fwd", "Cin2", "Cin = 2 not instantiated", Cin=2)
_refuse("chore_stem_x3_fwd", "Cin6", "Cin = 6 not instantiated", Cin=6)
_refuse("chore_absmax_f32", "n6", "absmax", n=6)
_refuse("chore_absmax_f32", "misaligned", "absmax", misalign=4)
_refuse("chore_absmax_f32", "null", "absmax", null=True)


# ================================================================================================ the coverage table
def _of(family, pred=lambda c: True):
    return [c["id"] for c in CASES[family] if pred(c)]


def _refused(fn):
    return _of("refused", lambda c: c["fn"] == fn)


COVERAGE = {
    "chore_gn_stats_bytes": "pure size function: every case with statistics gives its accumulators exactly this many bytes and a sentinel page",
    "chore_gn_stats": ids("gn_stats") + _of("gn_relu", lambda c: c["stats"] == "device") + _refused("chore_gn_stats"),
    "chore_gn_relu_fwd": ids("gn_relu") + _refused("chore_gn_relu_fwd"),
    "chore_avgpool2_fwd": ids("pool") + _refused("chore_avgpool2_fwd"),
    "chore_avgpool2_bwd": ids("pool_bwd") + _refused("chore_avgpool2_bwd"),
    "chore_upadd_fwd": ids("upadd") + _refused("chore_upadd_fwd"),
    "chore_up2_bwd": ids("up2_bwd") + _refused("chore_up2_bwd"),
    "chore_stem_workspace_bytes": "pure size function: every stem case gives the packed weights exactly this many bytes and a sentinel page",
    "chore_stem_fwd": ids("stem") + _refused("chore_stem_fwd"),
    "chore_stem_x3_workspace_bytes": "pure size function: every stem_x3 case gives the weight fragments exactly this many bytes and a sentinel page",
    "chore_stem_x3_fwd": ids("stem_x3") + _refused("chore_stem_x3_fwd"),
    "chore_amax_bytes": "pure size function: every absmax case gives the cells exactly this many bytes and a sentinel page",
    "chore_absmax_f32": ids("absmax") + _refused("chore_absmax_f32"),
}
# what no entry point reaches (only the encoder program of csrc/encoder.hip does), and where it stays covered
OUT_OF_SCOPE = {
    "gn_apply_relu_kernel<T, STATS = true>": "tests/test_gpu_encoder.py: the stem's GroupNorm writes tmpx and its statistics in one pass",
    "strided and offset Views (cs != C, co != 0)": "tests/test_gpu_encoder.py and tests/test_gpu_pool_fold.py: the ConvBlock slices of the encoder program",
    "the F16 instantiations of stem_kernel and map_stats_kernel<PoolOp>": "tests/test_gpu_encoder.py in the fp16 mode; the entry points refuse F16 (refused family)",
}
