"""The case matrix, the switch sets and the coverage table of tests/test_gpu_wgrad_kernels.py (no GPU needed to import this).

A case is one weight gradient as conv2d_bwd_weight_impl (csrc/train_bwd.hip) sees it: taps, input channels `cin`, output
channels `cout`, batch and map size, whether dbias is asked for, and a kind:
  "gn"     x random, GroupNorm + ReLU recomputed on it, dy random                 -> compared within the stated bounds
  "exact"  no GroupNorm, x and dy in {-1, 0, 1}                                   -> compared bit for bit
  "zero"   GroupNorm recomputed on a random x, dy == 0                            -> dW and dbias exactly 0
The shapes were chosen by reading wgrad_plan (the dispatch) and wgrad_shares / wgrad_shares_xcd (the share counts); which kernel each one
reaches is not asserted per case but through COVERAGE: every row marked to-reach must have been reported by
chore_debug_last_wgrad for at least one case of the run.

A coverage key is (kernel, element type, taps, mapping):
  kernel   "w32" wgrad_kernel, "w64" wgrad64_kernel, "w64x3" wgrad64_x3_kernel, "w64x3pc" wgrad64_x3_pc_kernel,
           "w128x3pc" wgrad128_x3_pc_kernel
  element  "fp32", "bf16", "x3": the arithmetic (an x3 layer below 64 channels runs the fp32 kernel and reports "fp32")
  mapping  how a workgroup finds its (share, channel pair): "grid" (wgrad_kernel: a 3-D grid), "xcd" (S % 8 == 0: shares
           interleaved over the XCDs) or "linear" in the 64- and 128-channel kernels; "gemm_tn" is wgrad_kernel<float, 1> as
           chore_gemm_tn_f32 launches it"""

MODES = ("fp32", "bf16", "x3")                  # _lib.F32, BF16, F16X3 in this order
KINDS = ("gn", "exact", "zero")
KERNELS = {1: "w32", 2: "w64", 3: "w64x3", 4: "w64x3pc", 5: "w128x3pc"}
CT = {"w32": 32, "w64": 64, "w64x3": 64, "w64x3pc": 64, "w128x3pc": 128}
FLAG_GN, FLAG_DBIAS, FLAG_XCD = 1, 2, 4
# the upstream gradient of the "gn" kind in x3 mode is N(0, 1) times one of these, by the position of the shape in SHAPES
X3_SCALES = (1e-7, 3e4, 1e-5, 1e2, 1e-3, 1.0, 1e-6, 1e4, 1e-1, 1e-4, 1e3, 1e-2)


def _c(name, taps, cin, cout, B, H, W, bias=False, poison=False):
    return dict(name=name, taps=taps, cin=cin, cout=cout, B=B, H=H, W=W, bias=bias, poison=poison)


# name, taps, cin, cout, B, H, W.  S and tiles below: 8-row tiles (w32, w64) / 4-row (w64x3) / 2-row (w64x3pc) / 32 pixels (w128x3pc)
SHAPES = [
    # ---- 3x3 ----
    _c("r64_64", 9, 64, 64, 2, 20, 44),                       # ragged in both axes; 12 / 20 tiles < S: S = tiles, linear (w64x3pc forced: 40, xcd)
    _c("t64_64", 9, 64, 64, 1, 3, 5, bias=True),              # a map smaller than one tile, S = 1
    _c("e256_128", 9, 256, 128, 2, 32, 64, poison=True),      # 8 pairs, S = 32, xcd: one 4-row tile per share (w64x3), two 2-row tiles (w64x3pc forced)
    _c("u256_128", 9, 256, 128, 3, 30, 40, bias=True),        # 48 4-row tiles over 32 shares: uneven; H % 4 != 0, W ragged, odd B
    _c("b128_64", 9, 128, 64, 3, 24, 96, bias=True),          # plain conv with bias; 27 / 54 / 108 tiles < S = 128: linear
    _c("n64_32", 9, 64, 32, 2, 24, 40, poison=True),          # the 32-channel kernel in every mode
    _c("n32_32", 9, 32, 32, 1, 5, 7, bias=True),              # ... on a map smaller than a tile
    _c("p128_128", 9, 128, 128, 1, 130, 127, bias=True, poison=True),   # H * W >= 128^2: w64x3pc<9> under DEFAULT dispatch, ragged in both axes, S = 64 xcd
    # ---- 1x1 ----
    _c("o64_128", 1, 64, 128, 2, 16, 32),                     # x3: w64x3pc<1> (Cin % 128 != 0), S = 16 xcd; forced w64x3<1>: S = 8 xcd
    _c("o128_256", 1, 128, 256, 2, 20, 44, poison=True),      # H * W % 32 != 0: w64x3pc<1>, not the 128 kernel; forced w64x3<1>: 20 tiles, linear
    _c("q128_128", 1, 128, 128, 1, 8, 32, bias=True),         # B H W = 256, the smallest the 128-channel kernel takes: S = 8 xcd
    _c("f128_128", 1, 128, 128, 1, 7, 32),                    # B H W = 224: falls through to w64x3pc<1>, 4 tiles, linear
    _c("l128_128", 1, 128, 128, 2, 12, 24, bias=True),        # H * W = 288 = 9 x 32 with W != 32: the 128 kernel on 18 tiles, linear
    _c("s256_256", 1, 256, 256, 2, 32, 64, bias=True, poison=True),   # the 128 kernel, S = 64 xcd, two tiles per share; w64<1>: S = 16 xcd
    _c("n32_96", 1, 32, 96, 2, 10, 12, bias=True),            # the 32-channel 1x1 kernel, bf16 included
]


def cases():
    out = []
    for i, s in enumerate(SHAPES):
        for kind in KINDS:
            c = dict(s)
            c["kind"] = kind
            c["id"] = s["name"] + "." + kind
            c["x3_scale"] = X3_SCALES[i % len(X3_SCALES)]
            out.append(c)
    return out


def uses64(case):
    """wgrad_use64 of train_bwd.hip for the 16-bit modes: below that the x3 mode runs the fp32 kernel whatever the switches say"""
    return case["cin"] % 64 == 0 and case["cout"] % 64 == 0


# switch set -> (environment, modes it is run in, taps it is run on (None: all), 64-channel shapes only)
SWITCH_SETS = {
    "default": ({}, MODES, None, False),
    "x3_v1": ({"CHORE_WGRAD_X3_V1": "1"}, ("x3",), None, True),          # wgrad64_x3_kernel on every 64-channel layer
    "x3_pc": ({"CHORE_WGRAD_X3_PC": "1"}, ("x3",), None, True),          # wgrad64_x3_pc_kernel on every one
    "no128": ({"CHORE_WGRAD_NO128": "1"}, ("x3",), (1,), True),          # the 1x1 layers without the 128-channel kernel
}
# the uninitialised-LDS check: the default set again on the shapes marked `poison`, with every CU's LDS filled with quiet NaNs
# after every launch of the library (CHORE_LDS_POISON, csrc/common.h)
POISON_ENV = {"CHORE_LDS_POISON": "0x7fc00000"}


def jobs_of(set_name):
    """[(case, mode)] a switch set runs"""
    _, modes, taps, only64 = SWITCH_SETS[set_name]
    out = []
    for c in cases():
        if (taps is not None and c["taps"] not in taps) or (only64 and not uses64(c)):
            continue
        out += [(c, m) for m in modes]
    return out


def witness_key(rec):
    """the coverage key of a chore_debug_last_wgrad record (kernel, element type, taps, ct, S, tiles, flags, launches)"""
    kern = KERNELS[int(rec[0])]
    assert int(rec[3]) == CT[kern], rec
    mapping = "grid" if kern == "w32" else ("xcd" if int(rec[6]) & FLAG_XCD else "linear")
    return (kern, MODES[int(rec[1])], int(rec[2]), mapping)


# ---- the coverage table: every instantiation the two launchers can pick, under each mapping ----
# (kernel, element type, taps) of the template instantiations launched from conv2d_bwd_weight_impl
INSTANTIATIONS = [("w32", "fp32", 1), ("w32", "fp32", 9), ("w32", "bf16", 1), ("w32", "bf16", 9), ("w64", "bf16", 1), ("w64", "bf16", 9),
                  ("w64x3", "x3", 1), ("w64x3", "x3", 9), ("w64x3pc", "x3", 1), ("w64x3pc", "x3", 9), ("w128x3pc", "x3", 1)]


def _coverage():
    t = {}
    for kern, dt, taps in INSTANTIATIONS:
        for mapping in (("grid",) if kern == "w32" else ("xcd", "linear")):
            t[(kern, dt, taps, mapping)] = None
    t[("w32", "fp32", 1, "gemm_tn")] = ("chore_gemm_tn_f32 is no convolution layer: test_gpu_bwd_operators.py::test_gemm_tn calls it against "
                                        "float64 and asserts this record of the witness itself")
    t[("any", "any", 0, "strided dy, deferred finish")] = (
        "not through chore_conv2d_bwd_weight: a channel-strided dy and wgrad_finish_multi_kernel exist only inside chore_convblock_bwd; "
        "tests/test_gpu_convblock_kernels.py compares all five kernels under them with float64 (tests/test_convblock_coverage_table.py)")
    return t


COVERAGE = _coverage()      # key -> None (the matrix must reach it) or the reason it does not
