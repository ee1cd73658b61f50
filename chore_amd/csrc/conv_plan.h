// conv_plan.h -- which kernel, tiling and flags a forward / data-gradient convolution gets: the one place that decides it
// ("Convolution forward: one launch plan").  Host arithmetic only: no handle, no device, no HIP header.  launch_conv
// (conv_lds.hip) forms the plan, notes it on the handle and switches on its family; the five launchers map it to a template
// instantiation; the encoder labels its profile classes from it; chore_conv_plan exports it for the CPU suite.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "../../include/chore_hip.h"

// kernel families and flag bits of a plan = of chore_handle::last_conv (include/chore_hip.h, chore_debug_last_conv)
enum { CONV_FAM_LDS = 1, CONV_FAM_SMALL = 2, CONV_FAM_PC = 3, CONV_FAM_MW = 4, CONV_FAM_RW = 5 };
enum { CONV_FLAG_SCALED = 1, CONV_FLAG_GN = 2, CONV_FLAG_SMALL_GRID = 4, CONV_FLAG_RES = 8, CONV_FLAG_POOL = 16 };
// the `fill` of the inference encoder's launches: half the CUs per launch, the other half for the other step in flight
constexpr int CONV_MW_FILL_INFER = 128;
// constants of the kernels that the choice depends on (each kernel file asserts that they are its own)
constexpr int CONV_LDS_TH = 8, CONV_LDS_TW = 32;   // conv_lds_kernel's tile
constexpr int CONV_LDS_PD_SMALL = 2;               // prefetch distance of its whole-chunk (small-grid) variant
constexpr int CONV_SMALL_PW = 34;                  // conv_small_kernel's patch row: 32 pixels + halo
constexpr int CONV_PROFILE_CLASSES = 27;           // conv_profile_class() < this

// what the choice depends on besides the shape
struct ConvTraits {
    bool gn = false;       // GroupNorm + ReLU fused into the input (ConvArgs::in_st)
    bool scaled = false;   // scaled operand: the fp16 x 3 data gradient (ConvArgs::in_amax)
    bool res = false, res2 = false, pool = false;   // residuals and pooled output present
    bool out = true;       // `out` present (a launch with a pooled output may leave it out)
    int fill = 0;          // ConvArgs::fill: 0, or CONV_MW_FILL_INFER
    int st_raw_C = 0, st_out_C = 0, st_pool_C = 0;   // channels of the tensors whose statistics the launch accumulates (0: none)
};
// chore_conv_plan's `traits_bits`
enum { CONV_TRAIT_GN = 1, CONV_TRAIT_SCALED = 2, CONV_TRAIT_RES = 4, CONV_TRAIT_RES2 = 8, CONV_TRAIT_POOL = 16, CONV_TRAIT_OUT = 32 };

// every A/B switch of the forward convolutions (DESIGN.md has the table), read ONCE per process: conv_switches() is the only instance
struct ConvSwitches {
    bool lds = getenv("CHORE_CONV_LDS") != nullptr;               // every layer on conv_lds_kernel or conv_small_kernel
    bool lds_bf16 = getenv("CHORE_CONV_LDS_BF16") != nullptr;     // bf16 never on conv_pc_kernel (rounds 1 - 4)
    bool pc_bf16 = getenv("CHORE_CONV_PC_BF16") != nullptr;       // bf16 on conv_pc_kernel wherever it has a tiling
    bool mw_off = getenv("CHORE_CONV_MW") && getenv("CHORE_CONV_MW")[0] == '0';      // conv_pc_kernel in conv_mw_kernel's place
    int mw_fill = getenv("CHORE_CONV_MW_FILL") ? atoi(getenv("CHORE_CONV_MW_FILL")) : 0;   // the `fill` of every launch (0: what it asks)
    bool mw_th2 = getenv("CHORE_CONV_MW_TH2") != nullptr;         // 2-row x 128-channel tiles for thin maps (experiment)
    bool rw_off = getenv("CHORE_CONV_RW") && atoi(getenv("CHORE_CONV_RW")) == 0;     // the 1x1 layers stay on conv_pc_kernel
    bool rw_x3only = getenv("CHORE_CONV_RW_X3ONLY") != nullptr;   // conv_rw_kernel's fp16 instantiation off
    bool rw_bf16 = getenv("CHORE_CONV_RW_BF16") != nullptr;       // ... its bf16 instantiation on (opt-in)
    bool no_small = getenv("CHORE_NO_CONV_SMALL") != nullptr;
    // conv_small_kernel's rows per workgroup by map size (-1: the default)
    int small_rows32 = getenv("CHORE_CONV_SMALL_ROWS32") ? atoi(getenv("CHORE_CONV_SMALL_ROWS32")) : -1;
    int small_rows64 = getenv("CHORE_CONV_SMALL_ROWS64") ? atoi(getenv("CHORE_CONV_SMALL_ROWS64")) : -1;
    int small_rows64_c256 = getenv("CHORE_CONV_SMALL_ROWS64_C256") ? atoi(getenv("CHORE_CONV_SMALL_ROWS64_C256")) : -1;
    const char* pc_force = getenv("CHORE_PC_FORCE");   // "taps,Cin,Cout,H:th*1000+nt[;...]" -- tiling experiments (scripts/conv_layer_ab.py)
};
inline const ConvSwitches& conv_switches() {
    static const ConvSwitches sw;
    return sw;
}

// exactly what a launcher needs to pick its instantiation; chore_debug_last_conv returns it field for field
struct ConvLaunchPlan {
    int family = 0;              // CONV_FAM_*
    int rows = 0;                // rows of a tile (conv_small_kernel: rows per workgroup; conv_rw_kernel: 0)
    int nt = 0;                  // output channels per workgroup
    int tps = 0, nslot = 0;      // taps per K-step; K-steps of weights resident in LDS (0: the kernel has no such ring)
    bool small_grid = false;     // conv_lds_kernel's whole-chunk variant (bit CONV_FLAG_SMALL_GRID of flags)
    int flags = 0;               // CONV_FLAG_*
    char refuse[160];            // why launch_conv refuses the arguments (its error text), or empty
    ConvLaunchPlan() { refuse[0] = 0; }
};

// ---- conv_pc_kernel / conv_mw_kernel: th rows x 32 pixels x nt channels per workgroup, tps taps per K-step, nslot K-steps of weights
// resident in LDS; th = 0: the layer has no tiling
struct ConvTile { int th, nt, tps, nslot; };

// taps per K-step and ring depth of a conv_pc tiling (what fits 160 KB of LDS)
// (measured, profiles/r03_conv_phase_breakdown.txt: rings of single taps with 4 - 6 slots are no faster than two slots of
// whole kernel rows -- the consumers pay per K-step for the hand-over -- except where only single taps fit: 128 channels)
inline ConvTile conv_pc_ring(int taps, int th, int nt) {
    if (taps == 1) return ConvTile{th, nt, 1, 2};
    if (nt == 128) return ConvTile{th, nt, 1, 3};
    if (th == 4 && nt == 32) return ConvTile{th, nt, 9, 2};
    return ConvTile{th, nt, 3, 2};
}
// tile configuration of the specialised-wave kernel for a layer.  force: th * 1000 + nt (development, e.g. 8064), 0: CHORE_PC_FORCE or the rule
inline ConvTile conv_pc_tile(int dtype, int taps, int B, int H, int W, int Cin, int Cout, const ConvSwitches& sw, int force = 0) {
    if ((dtype != CHORE_F16X3 && dtype != CHORE_F16 && dtype != CHORE_BF16) || Cin % 32 || Cout % 32) return ConvTile{0, 0, 0, 0};
    for (const char* q = force ? nullptr : sw.pc_force; q && *q;) {
        int t, ci, co, hh, f, n = 0;
        if (sscanf(q, "%d,%d,%d,%d:%d%n", &t, &ci, &co, &hh, &f, &n) == 5 && t == taps && ci == Cin && co == Cout && hh == H) { force = f; break; }
        while (*q && *q != ';') ++q;
        if (*q == ';') ++q;
    }
    if (force) return conv_pc_ring(taps, force / 1000, force % 1000);
    const long px_tiles8 = (long)B * ((H + 7) / 8) * (W / 32);
    if (taps == 1) {
        if (Cout % 128 == 0) return conv_pc_ring(1, 8, 128);
        if (Cout % 64 == 0) return conv_pc_ring(1, 8, 64);
        return ConvTile{0, 0, 0, 0};
    }
    // 3x3: the widest channel tile that still gives every CU a workgroup; 4-row tiles when 8-row tiles leave CUs idle
    if (Cout % 128 == 0 && px_tiles8 * (Cout / 128) >= 256) return conv_pc_ring(9, 8, 128);
    if (Cout % 64 == 0 && px_tiles8 * (Cout / 64) >= 256) return conv_pc_ring(9, 8, 64);
    if (px_tiles8 * (Cout / 32) >= 256) return conv_pc_ring(9, 8, 32);
    if (H % 4 == 0 && Cout % 64 == 0 && px_tiles8 * 2 * (Cout / 64) >= 256) return conv_pc_ring(9, 4, 64);
    if (H % 4 == 0) return conv_pc_ring(9, 4, 32);
    return conv_pc_ring(9, 8, 32);
}

// conv_mw_kernel (the same tilings with the staging inside the MFMA-issuing waves): by mode -- fp16 x 3, 3x3, not switched off
inline bool conv_mw_on(int dtype, int taps, const ConvSwitches& sw) { return !sw.mw_off && dtype == CHORE_F16X3 && taps == 9; }
// the `fill` a launch gets: CHORE_CONV_MW_FILL if set (every launch), else what it asks (0 -> 256: a tile per CU)
inline int conv_mw_fill(int asked, const ConvSwitches& sw) { return sw.mw_fill > 0 ? sw.mw_fill : (asked > 0 ? asked : 256); }
// The tiling for a layer: conv_pc_tile's.  CHORE_CONV_MW_TH2=1 (experiment, measured equal: 256 -> 128 at 64^2, B = 4, 41.5 - 42.4 us
// against 40.6 - 42.4, profiles/r06_conv_layer_ab.txt): 128 output channels on maps with fewer than 256 eight-row tiles as
// 2 x 32 pixels x 128 channels (0.4 of the 256-channel patch staged once) instead of four 32-channel workgroups per 8 x 32 pixels
// that each stage the whole patch -- the staging is not what bounds that layer
inline ConvTile conv_mw_tile(int dtype, int taps, int B, int H, int W, int Cin, int Cout, int fill_asked, const ConvSwitches& sw) {
    ConvTile p = conv_pc_tile(dtype, taps, B, H, W, Cin, Cout, sw);
    if (sw.mw_th2 && p.th && taps == 9 && Cout % 128 == 0 && p.nt < 128 && H % 2 == 0) {
        const long tiles2 = (long)B * (H / 2) * ((W + 31) / 32) * (Cout / 128);
        if (tiles2 >= 256) p = ConvTile{2, 128, 1, 3};
    }
    // A layer too small to give every CU a full tile (the 64^2 and 32^2 maps at B = 4) takes the WIDEST tile that still yields
    // `fill` workgroups (ConvArgs::fill; the inference encoder asks for 128 = half the CUs) instead of the narrowest that yields 256 -- fewer, denser workgroups:
    // the same launch time on half of the CUs, the other half free for the other step in flight (two in flight 4.24 -> 3.99 ms, one
    // at a time 5.03 -> 5.06; 64: 4.03 / 5.47; profiles/r06_conv_fill.txt).  Also takes the 32^2 maps over from conv_small_kernel.
    // CHORE_CONV_MW_FILL=256: a tile per CU as conv_pc_tile has it.
    const int fill = conv_mw_fill(fill_asked, sw);
    if (fill < 256 && conv_mw_on(dtype, taps, sw) && Cin % 32 == 0 && W % 32 == 0) {
        const long px8 = (long)B * ((H + 7) / 8) * (W / 32);
        if (px8 * (Cout / 32) < 256 || !p.th || (p.th == 4 && p.nt == 32) || (p.th == 8 && p.nt == 32 && px8 * (Cout / 32) < 512)) {
            static const ConvTile cand[] = {{8, 128, 1, 3}, {4, 128, 1, 3}, {2, 128, 1, 3}, {8, 64, 3, 2}, {4, 64, 3, 2}, {2, 64, 1, 3},
                                            {8, 32, 3, 2}, {4, 32, 9, 2}};
            for (const ConvTile& c : cand) {
                if (Cout % c.nt || H % c.th) continue;
                if ((long)B * (H / c.th) * (W / 32) * (Cout / c.nt) >= fill) { p = c; break; }
            }
        }
    }
    return p;
}
// an instantiation of conv_mw_kernel exists for this tiling (the MW_CASE lines of conv_mw.hip) and for these arguments: the
// GroupNorm-fused forward or the scaled data gradient, no second residual
inline bool conv_mw_covers(const ConvTile& p, const ConvTraits& t) {
    const int key = (p.th * 1000 + p.nt) * 100 + p.tps * 10 + p.nslot;
    return !t.res2 && t.gn != t.scaled &&
           (key == 812813 || key == 806432 || key == 803232 || key == 406432 || key == 403292 || key == 212813 || key == 412813 || key == 206413);
}

// A launch of this layer can carry a pooled output (ConvArgs::pool): by mode, taps, channels and even H and W -- never by the batch
// size (one image alone and the same image inside a batch must take the same path).  conv_mw_kernel only, and every tiling
// conv_mw_tile yields pools (conv_pc_tile's fall-through is 8 or 4 rows x 32 channels); the 1x1 layers keep the pooling pass
// (DESIGN section 4).  Callers ask before they build their ConvArgs; launch_conv refuses a pooled output elsewhere.
inline bool conv_pool_covers(int dtype, int taps, int Cin, int Cout, int H, int W, const ConvSwitches& sw = conv_switches()) {
    return !sw.lds && conv_mw_on(dtype, taps, sw) && Cin % 32 == 0 && Cin <= 256 && Cout % 32 == 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0;
}

// ---- conv_small_kernel (small maps: one workgroup = rows x 32 pixels x 32 output channels, K split over its four waves)
// rows per workgroup; 0 = not this kernel.  The larger maps default to 0; the switches override for A/B measurements.
inline int conv_small_rows(int dtype, int H, int W, int Cin, const ConvSwitches& sw) {
    const bool x3 = dtype == CHORE_F16X3;
    int rows;
    if (H * W <= 32 * 32) rows = sw.small_rows32 >= 0 ? sw.small_rows32 : ((x3 || dtype == CHORE_F16) ? 2 : 1);
    else if (Cin == 256) rows = sw.small_rows64_c256 >= 0 ? sw.small_rows64_c256 : 0;
    else rows = sw.small_rows64 >= 0 ? sw.small_rows64 : 0;
    // LDS: (rows + 2) x 34 pixels x (2 Cin + 16) bytes per plane, two planes for fp16 x 3
    while (rows > 0 && (size_t)(x3 ? 2 : 1) * (rows + 2) * CONV_SMALL_PW * (Cin * 2 + 16) + (size_t)Cin * 8 + 2048 > 160 * 1024) rows >>= 1;
    if (rows && H % rows) rows = 0;
    return rows;
}
// Where it is used (measured, bench.py encode time, B = 4: bf16 4.06 -> 3.79 ms, fp16 x 3 6.55 -> 6.1 ms).  A workgroup
// fetches its K slice of the weights (147 KB for 256 -> 128 channels) and its halo patch from L2 on its own, so the
// kernel trades L2 traffic for parallelism.  It wins on the 32 x 32 maps, where conv_lds_kernel has 16-64 workgroups for
// 256 CUs.  On the 64 x 64 maps it loses in every variant tried (1, 2 or 4 rows per workgroup, CHORE_CONV_SMALL_ROWS64*):
// 1 024-2 048 workgroups x 200 KB is L2-bandwidth bound (53 us against 26 us for the 256-channel convolution), and with
// several rows per workgroup the waves drift apart and each pulls the weight fragments through the 32 KB L1 again --
// sharing them takes the LDS ring and barriers of conv_lds_kernel, which therefore keeps those maps.  bf16, fp16 and
// fp16 x 3 only: the native-fp32 parity mode keeps the one kernel it was validated with.
inline bool conv_small_eligible(int dtype, int taps, int H, int W, int Cin, int Cout, const ConvSwitches& sw) {
    if (sw.no_small || taps != 9 || (dtype != CHORE_BF16 && dtype != CHORE_F16X3 && dtype != CHORE_F16)) return false;
    if (W % 32 || Cout % 32 || (Cin != 64 && Cin != 128 && Cin != 256) || H * W > 64 * 64) return false;
    return conv_small_rows(dtype, H, W, Cin, sw) > 0;
}

// ---- conv_rw_kernel: 1x1 layers (fp16 x 3, fp16, bf16) with register-resident weights, by shape (the RW_CASE lines of conv_rw.hip)
// bf16 is OPT-IN (CHORE_CONV_RW_BF16=1): alone the layers are faster (256 -> 256 at 128^2 24.8 against 36.2 us on conv_lds_kernel), inside the
// encoder they are not (12 launches: 0.399 against 0.376 ms per step; whole bf16 step 3.28 against 3.25 ms, profiles/r05_conv_rw.txt):
// conv_lds_kernel's many small workgroups hide a cold start (weights, statistics, instructions) that one persistent workgroup
// per CU pays in full on a 20 us kernel.
inline bool conv_rw_covers(int dtype, int taps, int Cin, int Cout, bool scaled, const ConvSwitches& sw) {
    if (sw.rw_off || taps != 1 || (dtype != CHORE_F16X3 && dtype != CHORE_F16 && dtype != CHORE_BF16)) return false;
    if (dtype == CHORE_F16 && sw.rw_x3only) return false;
    if (dtype == CHORE_BF16 && !sw.rw_bf16) return false;
    if (scaled) return dtype == CHORE_F16X3 && Cin == 256 && Cout == 256;     // data gradients of fp16 x 3 training: the stack tail's layers
    return (Cin == 256 && Cout == 256) || (Cin == 128 && Cout == 256) || (Cin == 64 && Cout == 128);
}

// ---- conv_lds_kernel: 8 x 32 pixels x nt channels
inline long conv_lds_tiles(int H, int W) { return (long)((W + CONV_LDS_TW - 1) / CONV_LDS_TW) * ((H + CONV_LDS_TH - 1) / CONV_LDS_TH); }
// N-tile choice: the largest channel tile that still gives every CU about two workgroups
inline int conv_lds_nt(int dtype, int B, int H, int W, int Cout) {
    int best = 32;
    long best_wgs = -1;
    for (int nt : {128, 64, 32}) {
        if (Cout % nt) continue;
        if (nt == 128 && dtype != CHORE_BF16) continue;  // the 4x2 register tile fits 256 VGPRs with bf16 operands only
        const long wgs = (long)B * conv_lds_tiles(H, W) * (Cout / nt);
        if (wgs >= 448) return nt;
        if (wgs > best_wgs) { best_wgs = wgs; best = nt; }
    }
    return best;
}
// small grid: fewer workgroups than 1.5 per CU -> whole-chunk K-steps with deep register prefetch (needs the chunk count to be a
// multiple of the prefetch distance; not fp16 x 3: two LDS planes per operand, the whole-chunk variant would not fit)
inline bool conv_lds_small_grid(int dtype, int B, int H, int W, int Cin, int Cout, int nt) {
    if (dtype == CHORE_F16X3) return false;
    const int nch = Cin / (dtype == CHORE_F32 ? 16 : 32);
    return nt <= 64 && nch % CONV_LDS_PD_SMALL == 0 && (long)B * conv_lds_tiles(H, W) * (Cout / nt) < 384;
}

inline bool conv_gn_group_ok(int channels) {      // GroupNorm(32, channels): group size 1, 2, 4 or 8
    const int gs = channels / 32;
    return channels % 32 == 0 && gs <= 8 && !(gs & (gs - 1));
}

// The plan of a launch: the first rule that matches, in this order (DESIGN.md has the table)
inline ConvLaunchPlan conv_launch_plan(int dtype, int taps, int B, int H, int W, int Cin, int Cout, const ConvTraits& t,
                                       const ConvSwitches& sw) {
    ConvLaunchPlan p;
    p.flags = (t.scaled ? CONV_FLAG_SCALED : 0) | (t.gn ? CONV_FLAG_GN : 0) | (t.res ? CONV_FLAG_RES : 0) | (t.pool ? CONV_FLAG_POOL : 0);
#define CONV_REFUSE(...) do { snprintf(p.refuse, sizeof(p.refuse), __VA_ARGS__); return p; } while (0)
    auto tiled = [&p](int family, const ConvTile& tile) {
        p.family = family; p.rows = tile.th; p.nt = tile.nt; p.tps = tile.tps; p.nslot = tile.nslot;
        return p;
    };
    if (dtype != CHORE_F32 && dtype != CHORE_BF16 && dtype != CHORE_F16X3 && dtype != CHORE_F16) CONV_REFUSE("conv: bad dtype");
    if (Cin % (dtype == CHORE_F32 ? 16 : 32) || Cin > 256) CONV_REFUSE("conv: unsupported Cin=%d", Cin);
    if (Cout % 32) CONV_REFUSE("conv: unsupported Cout=%d", Cout);
    if (B > 65535) CONV_REFUSE("conv: B too large");
    if (taps != 1 && taps != 9) CONV_REFUSE("conv: taps must be 1 or 9");
    for (int c : {t.st_raw_C ? t.st_raw_C : 32, t.st_out_C ? t.st_out_C : 32, t.gn ? Cin : 32, t.pool && t.st_pool_C ? t.st_pool_C : 32})
        if (!conv_gn_group_ok(c)) CONV_REFUSE("conv: GroupNorm over %d channels unsupported (group size must be 1, 2, 4 or 8)", c);
    const ConvTile mp = conv_mw_on(dtype, taps, sw) ? conv_mw_tile(dtype, taps, B, H, W, Cin, Cout, t.fill, sw) : ConvTile{0, 0, 0, 0};
    const bool mw = mp.th && conv_mw_covers(mp, t);      // conv_mw_kernel can take the launch
    if (t.pool) {   // a pooled output rides in conv_mw_kernel's epilogue only: the caller asked conv_pool_covers() first
        if (!conv_pool_covers(dtype, taps, Cin, Cout, H, W, sw) || !mw)
            CONV_REFUSE("conv: this launch cannot carry a pooled output (taps=%d Cin=%d Cout=%d %dx%d)", taps, Cin, Cout, H, W);
        if (t.scaled) CONV_REFUSE("conv_mw: no pooled output on the data-gradient kernels");
        return tiled(CONV_FAM_MW, mp);
    }
    if (!t.out) CONV_REFUSE("conv: no output");
    // the small maps on dense conv_mw tiles (conv_mw_tile) come before conv_small_kernel
    if (mw && conv_mw_fill(t.fill, sw) < 256) return tiled(CONV_FAM_MW, mp);
    if (conv_small_eligible(dtype, taps, H, W, Cin, Cout, sw)) return tiled(CONV_FAM_SMALL, ConvTile{conv_small_rows(dtype, H, W, Cin, sw), 32, 9, 0});
    // 1x1 (every 16-bit-operand mode): weights resident in registers, persistent workgroups (fp16 x 3 256 -> 256 at 128^2: 64 -> 39 us)
    if (!t.res2 && !sw.lds && conv_rw_covers(dtype, taps, Cin, Cout, t.scaled, sw)) return tiled(CONV_FAM_RW, ConvTile{0, Cout, 1, 0});
    const ConvTile pp = conv_pc_tile(dtype, taps, B, H, W, Cin, Cout, sw);
    if (dtype == CHORE_F16) {   // fp16 tensors: the specialised-wave kernel is the only implementation
        if (!pp.th || t.res2) CONV_REFUSE("conv: layer not covered in the fp16 mode (Cin=%d Cout=%d)", Cin, Cout);
        return tiled(CONV_FAM_PC, pp);
    }
    // specialised-wave kernels: fp16 x 3; since round 5 also bf16, where conv_pc_kernel measured faster layer by layer
    // (profiles/r05_conv_layer_ab.txt: 3x3 layers of <= 128 input channels on maps up to 128^2 -- 64^2 128->64 15.4 against 20.2 us,
    // 64->64 13.2 against 15.7; the 1x1 layers, the 256-channel inputs and the 256^2 maps stay on conv_lds_kernel, which wins there:
    // with one MFMA per product the bf16 K loop is short and the producer / consumer hand-over costs more than it hides)
    const bool bf16_pc = dtype == CHORE_BF16 && !sw.lds_bf16 && (sw.pc_bf16 || (taps == 9 && Cin <= 128 && (long)H * W <= 128 * 128));
    if ((dtype == CHORE_F16X3 || bf16_pc) && !t.res2 && !sw.lds) {
        if (mw) return tiled(CONV_FAM_MW, mp);
        if (pp.th) return tiled(CONV_FAM_PC, pp);
    }
    const int nt = conv_lds_nt(dtype, B, H, W, Cout);
    p.small_grid = conv_lds_small_grid(dtype, B, H, W, Cin, Cout, nt);
    if (p.small_grid) p.flags |= CONV_FLAG_SMALL_GRID;
    return tiled(CONV_FAM_LDS, ConvTile{CONV_LDS_TH, nt, taps == 1 ? 1 : (p.small_grid ? 9 : 3), 2});
#undef CONV_REFUSE
}

// the encoder's profile class of a plan, counted from its first convolution class (encoder.hip: kclass_names from K_CONV_FIRST on)
inline int conv_profile_class(const ConvLaunchPlan& p, int taps, int Cin) {
    const int ni = p.nt == 128 ? 0 : (p.nt == 64 ? 1 : 2);
    switch (p.family) {
    case CONV_FAM_SMALL: return 8 + (Cin == 64 ? 0 : (Cin == 128 ? 1 : 2));
    case CONV_FAM_PC: return 11 + (taps == 1 ? (p.nt == 128 ? 5 : 6) : (p.rows == 8 ? ni : (p.nt == 64 ? 3 : 4)));
    case CONV_FAM_RW: return 18;
    case CONV_FAM_MW: return 19 + (p.rows == 8 ? ni : (p.rows == 4 ? (p.nt == 128 ? 6 : (p.nt == 64 ? 3 : 4)) : (p.nt == 128 ? 5 : 7)));
    default: return taps == 1 ? 5 + ni : (p.tps == 9 ? 3 + (ni > 0 ? ni - 1 : 0) : ni);
    }
}
