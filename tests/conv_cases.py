"""The case matrix, the switch sets and the coverage table of tests/test_gpu_conv_kernels.py (no GPU needed to import this).

A case is one convolution as launch_conv (csrc/conv_lds.hip) sees it: taps, input channels `cin`, output channels `cout`, batch
and map size, and a kind:
  "gn"     forward with GroupNorm + ReLU fused into the input, random values      -> compared within the stated bounds
  "plain"  forward without GroupNorm, inputs and weights in {-1, 0, 1}            -> compared bit for bit
  "bwd"    data gradient (chore_conv2d_bwd_data: dy has `cin` channels, dx `cout`; the layer's weight is (cin, cout, k, k)),
           inputs and weights in {-1, 0, 1}                                        -> compared bit for bit
The shapes were chosen by reading the planners (csrc/conv_plan.h: conv_pc_tile, conv_mw_tile, conv_small_rows, conv_rw_covers, conv_lds_nt,
conv_lds_small_grid); which kernel each one reaches is pinned job by job in tests/conv_plan_cases.py (EXPECTED) and summed up in
COVERAGE: every row marked covered must have been reported by chore_debug_last_conv for at least one case of the run.

A coverage key names one template instantiation a launcher can pick:
  ("pc", dtype, taps, th, nt, tps, nslot)     conv_pc_kernel, the PC_CASE lines;   dtype: "fp16", "bf16", "x3", "x3s"
  ("mw", variant, th, nt, tps, nslot)         conv_mw_kernel, the MW_CASE lines;   variant: "gn" (GroupNorm-fused forward), "scaled"
  ("rw", dtype, cin, cout, res)               conv_rw_kernel, the RW_CASE shapes;  res: "" or "res"
  ("small", dtype, cin, rows)                 conv_small_kernel
  ("lds", dtype, taps, nt, small_grid)        conv_lds_kernel;                     dtype: "fp32", "bf16", "x3", "x3s"
"x3s" is the scaled-input variant of fp16 x 3 (the data gradient, ConvArgs::in_amax)."""

MODES = ("fp32", "bf16", "x3", "fp16")          # _lib.F32, BF16, F16X3, F16 in this order
FAMILIES = {1: "lds", 2: "small", 3: "pc", 4: "mw", 5: "rw"}
FLAG_SCALED, FLAG_GN, FLAG_SMALL_GRID, FLAG_RES = 1, 2, 4, 8


def _c(name, taps, cin, cout, B, H, W, kinds, bias=False, modes=MODES, poison=False, only=None):
    return dict(name=name, taps=taps, cin=cin, cout=cout, B=B, H=H, W=W, kinds=kinds, bias=bias, modes=tuple(modes), poison=poison,
                only=only)


# name, taps, cin, cout, B, H, W, kinds.  `only`: switch sets the shape is run in (None: every set that takes its taps and modes)
SHAPES = [
    # ---- 3x3, the production shapes: B = 4 on 128^2, 64^2 and 32^2 maps ----
    _c("p256_128", 9, 256, 128, 4, 128, 128, ("gn",), poison=True),          # 8 x 32 x 128; fp32 / bf16: conv_lds nt 64
    _c("p128_128", 9, 128, 128, 4, 128, 128, ("plain", "bwd")),              # ... the exact cases of that tiling
    _c("p128_64", 9, 128, 64, 4, 128, 128, ("gn", "plain", "bwd"), bias=True),   # 8 x 32 x 64
    _c("p64_32", 9, 64, 32, 4, 128, 128, ("gn", "plain", "bwd")),            # 8 x 32 x 32; conv_lds nt 32 small grid
    _c("m64_64", 9, 64, 64, 4, 64, 64, ("gn", "plain", "bwd"), bias=True, poison=True),     # 4 x 32 x 32; dense, pc_force: 4 x 32 x 64
    _c("m64_64r", 9, 64, 64, 3, 64, 40, ("gn", "plain", "bwd"), only=("pc_force",)),   # pc_force: 4 x 32 x 64 with a ragged W, odd B
    _c("m256_128", 9, 256, 128, 4, 64, 64, ("gn", "bwd")),                   # 8 x 32 x 32; dense: 4 x 32 x 128; TH2: 2 x 32 x 128
    _c("m128_128", 9, 128, 128, 2, 64, 64, ("gn", "plain", "bwd")),          # 4 x 32 x 32; dense: 2 x 32 x 128
    _c("s256_128", 9, 256, 128, 4, 32, 32, ("gn", "plain", "bwd"), bias=True, poison=True),   # conv_small Cin 256; dense: 2 x 32 x 64
    _c("s128_64", 9, 128, 64, 4, 32, 32, ("gn", "plain", "bwd"), bias=True),     # conv_small Cin 128
    _c("s64_64", 9, 64, 64, 3, 30, 32, ("gn", "plain", "bwd"), bias=True),   # conv_small Cin 64, odd B, H not a multiple of 4
    _c("sr128_32", 9, 128, 32, 3, 30, 32, ("gn", "plain", "bwd")),           # conv_small Cin 128, ragged the same way
    _c("sr256_64", 9, 256, 64, 5, 22, 32, ("gn", "plain", "bwd")),           # conv_small Cin 256, odd B, H not a multiple of 4
    # ---- 3x3, ragged: H not a multiple of the tile's rows, W not a multiple of 32, maps smaller than a tile, odd B ----
    _c("r32_128", 9, 32, 128, 5, 100, 136, ("gn", "plain", "bwd"), bias=True),   # 8 x 32 x 128; conv_lds nt 64
    _c("r32_64", 9, 32, 64, 5, 100, 136, ("gn", "bwd")),                     # 8 x 32 x 64
    _c("r32_32", 9, 32, 32, 5, 100, 136, ("gn", "plain", "bwd"), bias=True),     # 8 x 32 x 32; bf16 conv_lds nt 32, not small (one chunk)
    _c("t128_64", 9, 128, 64, 3, 20, 28, ("gn", "plain", "bwd")),            # 4 x 32 x 32 on a map narrower than a tile
    _c("t64_32", 9, 64, 32, 3, 22, 28, ("gn", "plain", "bwd"), bias=True),   # 8 x 32 x 32 (H % 4 != 0) on such a map
    _c("h64_128", 9, 64, 128, 5, 54, 40, ("gn", "bwd")),                     # TH2: 2 x 32 x 128 with a ragged W
    _c("d4x128", 9, 64, 128, 3, 44, 128, ("gn", "bwd"), bias=True),                    # dense: 4 x 32 x 128, H % 8 != 0, odd B
    _c("d2x128", 9, 64, 128, 3, 46, 64, ("gn", "bwd"), bias=True),                    # dense: 2 x 32 x 128, H % 4 != 0
    _c("d2x64", 9, 64, 64, 3, 46, 64, ("gn", "bwd"), bias=True),             # dense: 2 x 32 x 64
    _c("d4x64", 9, 64, 64, 3, 44, 128, ("gn", "bwd"), bias=True),                    # dense: 4 x 32 x 64
    # ---- conv_lds_kernel's widest channel tile (bf16 only: 128 channels per workgroup need >= 448 workgroups) ----
    _c("n32_256", 9, 32, 256, 4, 128, 128, ("gn",), bias=True, modes=("bf16",), only=("default", "lds_bf16")),
    _c("n32_256r", 9, 32, 256, 5, 100, 136, ("gn", "plain"), modes=("bf16",), only=("default", "lds_bf16")),   # ... ragged: 650 workgroups
    _c("v32_256r", 1, 32, 256, 5, 100, 136, ("gn", "plain"), modes=("bf16",), only=("default", "lds_bf16")),   # ... and its 1x1 form
    # ---- 1x1 ----
    _c("w256_256", 1, 256, 256, 4, 128, 128, ("gn", "bwd"), bias=True, poison=True),   # conv_rw 256 -> 256 and its scaled data gradient; bf16: conv_lds nt 128
    _c("w256_256r", 1, 256, 256, 3, 20, 44, ("plain", "bwd"), bias=True),            # ... ragged, exact
    _c("w128_256", 1, 128, 256, 3, 20, 44, ("gn", "plain"), bias=True),      # conv_rw 128 -> 256, ragged
    _c("w128_256p", 1, 128, 256, 4, 64, 64, ("gn",)),                        # ... production
    _c("w64_128", 1, 64, 128, 4, 128, 128, ("gn", "plain"), bias=True),      # conv_rw 64 -> 128
    _c("w64_128r", 1, 64, 128, 3, 20, 44, ("gn", "plain")),                  # ... ragged
    _c("o128_128", 1, 128, 128, 3, 24, 40, ("gn", "plain", "bwd"), bias=True),   # conv_pc 1x1 8 x 32 x 128
    _c("o64_64", 1, 64, 64, 7, 128, 128, ("gn", "plain", "bwd"), bias=True, poison=True),  # conv_pc 1x1 8 x 32 x 64; conv_lds nt 64
    _c("o64_64r", 1, 64, 64, 7, 100, 136, ("gn", "plain", "bwd")),           # ... ragged, still the 448 workgroups of conv_lds nt 64
    _c("o64_32", 1, 64, 32, 2, 16, 32, ("gn", "plain", "bwd"), modes=("fp32", "bf16", "x3")),   # no conv_pc tiling: conv_lds in fp16 x 3
]


def cases():
    out = []
    for s in SHAPES:
        for kind in s["kinds"]:
            c = dict(s)
            c["kind"] = kind
            c["id"] = s["name"] + "." + kind
            del c["kinds"]
            out.append(c)
    return out


# switch set -> (environment, modes it is run in, taps it is run on (None: all), kinds (None: all), shapes (None: all))
SWITCH_SETS = {
    "default": ({}, MODES, None, None, None),
    "mw0": ({"CHORE_CONV_MW": "0"}, ("x3",), (9,), None, None),                                 # conv_pc in fp16 x 3
    "fill128": ({"CHORE_CONV_MW_FILL": "128"}, ("x3",), (9,), ("gn", "bwd"), None),              # the dense conv_mw tilings
    "fill256_th2": ({"CHORE_CONV_MW_FILL": "256", "CHORE_CONV_MW_TH2": "1"}, ("x3",), (9,), ("gn", "bwd"), None),
    "no_small": ({"CHORE_NO_CONV_SMALL": "1"}, ("bf16", "x3", "fp16"), (9,), None, ("s256_128", "s128_64", "s64_64")),
    "rw0": ({"CHORE_CONV_RW": "0"}, ("x3", "fp16"), (1,), None, None),
    "lds": ({"CHORE_CONV_LDS": "1"}, ("x3",), None, None, None),                                # fp16 x 3 and the scaled gradient on conv_lds
    "pc_bf16": ({"CHORE_CONV_PC_BF16": "1"}, ("bf16",), None, None, None),
    "lds_bf16": ({"CHORE_CONV_LDS_BF16": "1"}, ("bf16",), None, None, None),
    "rw_bf16": ({"CHORE_CONV_RW_BF16": "1"}, ("bf16",), (1,), None, None),
    # an experiment switch, cheap to cover: conv_pc_tile never picks 4 x 32 x 64 by itself (its condition equals the one of
    # 8 x 32 x 32, which is tested first), CHORE_PC_FORCE puts the 64 -> 64 layers of the 64^2 map on it
    "pc_force": ({"CHORE_CONV_MW": "0", "CHORE_PC_FORCE": "9,64,64,64:4064"}, ("bf16", "x3", "fp16"), (9,), None, ("m64_64", "m64_64r")),
}
# the uninitialised-LDS check: the default set again, one case per family, with every CU's LDS filled with quiet NaNs after
# every launch of the library (CHORE_LDS_POISON, csrc/common.h).  The pattern is given explicitly: "1" would be taken as the
# pattern 0x00000001, a denormal that an fp32 addition swallows
POISON_ENV = {"CHORE_LDS_POISON": "0x7fc00000"}


def jobs_of(set_name):
    """[(case, mode)] a switch set runs"""
    _, modes, taps, kinds, shapes = SWITCH_SETS[set_name]
    out = []
    for c in cases():
        if c["only"] is not None and set_name not in c["only"]:
            continue
        if shapes is not None and c["name"] not in shapes:
            continue
        if (taps is not None and c["taps"] not in taps) or (kinds is not None and c["kind"] not in kinds):
            continue
        out += [(c, m) for m in modes if m in c["modes"]]
    return out


def witness_key(case, mode, rec):
    """the coverage key of a chore_debug_last_conv record (family, rows, nt, tps, nslot, flags, cin, launches)"""
    fam = FAMILIES[int(rec[0])]
    rows, nt, tps, nslot, flags = (int(v) for v in rec[1:6])
    scaled = bool(flags & FLAG_SCALED)
    dt = ("x3s" if scaled else "x3") if mode == "x3" else mode
    if fam == "pc":
        return ("pc", dt, case["taps"], rows, nt, tps, nslot)
    if fam == "mw":
        return ("mw", "scaled" if scaled else "gn", rows, nt, tps, nslot)
    if fam == "rw":
        return ("rw", dt, case["cin"], case["cout"], "res" if flags & FLAG_RES else "")
    if fam == "small":
        return ("small", dt, case["cin"], rows)
    # (a 1x1 layer has no small-grid variant: launch_nt ignores the flag there)
    return ("lds", dt, case["taps"], nt, case["taps"] == 9 and bool(flags & FLAG_SMALL_GRID))


# ---- the coverage table: every instantiation the launchers can pick, covered by the matrix or not (with the reason) ----
PC_TILINGS = [(9, 8, 128, 1, 3), (9, 8, 64, 3, 2), (9, 8, 32, 3, 2), (9, 4, 64, 3, 2), (9, 4, 32, 9, 2), (1, 8, 128, 1, 2), (1, 8, 64, 1, 2)]
MW_TILINGS = [(8, 128, 1, 3), (4, 128, 1, 3), (2, 128, 1, 3), (2, 64, 1, 3), (8, 64, 3, 2), (8, 32, 3, 2), (4, 64, 3, 2), (4, 32, 9, 2)]
RW_SHAPES = [(256, 256), (128, 256), (64, 128)]
SMALL_ROWS = (1, 2, 4)
SMALL_DEFAULT_ROWS = {"bf16": 1, "x3": 2, "fp16": 2, "x3s": 2}       # conv_small_rows() of a process without CHORE_CONV_SMALL_ROWS*


def _coverage():
    t = {}
    for tiling in PC_TILINGS:
        for dt in ("fp16", "bf16", "x3", "x3s"):
            t[("pc", dt) + tiling] = None
    for tiling in MW_TILINGS:
        for v in ("gn", "scaled"):
            t[("mw", v) + tiling] = None
    for dt in ("x3", "fp16", "bf16"):
        for cin, cout in RW_SHAPES:
            t[("rw", dt, cin, cout, "")] = None
            t[("rw", dt, cin, cout, "res")] = "a residual reaches conv_rw_kernel only from the encoder program (test_encoder_512_checksums)"
    t[("rw", "x3s", 256, 256, "")] = None
    t[("rw", "x3s", 256, 256, "res")] = ("instantiated, but no caller launches it: no data gradient carries a residual, and the ConvBlock operator's only "
                                         "1x1 data gradient has Cin != Cout (tests/test_convblock_coverage_table.py holds both)")
    for dt, dflt in SMALL_DEFAULT_ROWS.items():
        for cin in (64, 128, 256):
            for rows in SMALL_ROWS:
                t[("small", dt, cin, rows)] = None if rows == dflt else "only the experiment switches CHORE_CONV_SMALL_ROWS* pick these rows"
    for dt, nts in (("fp32", (64, 32)), ("bf16", (128, 64, 32))):
        for nt in nts:
            t[("lds", dt, 1, nt, False)] = None
            t[("lds", dt, 9, nt, False)] = None
        t[("lds", dt, 9, 32, True)] = None
        t[("lds", dt, 9, 64, True)] = ("unreachable: conv_lds_nt returns 64 only from 448 workgroups on, the small-grid variant needs "
                                       "fewer than 384")
    for dt in ("x3", "x3s"):
        for taps in (1, 9):
            for nt in (64, 32):
                t[("lds", dt, taps, nt, False)] = None
    return t


COVERAGE = _coverage()      # key -> None (the matrix must reach it) or the reason it does not
