// query_plan.h -- which kernel a query call runs: the one place that decides it ("Query: one launch plan").
// Host arithmetic only: no handle, no device, no HIP call.  capi.hip forms the plan, launch_query_fwd (query_fwd.hip) and
// launch_query_bwd (query_bwd.hip) map it to an instantiation, chore_query_plan exports it for the CPU suite.
#pragma once
#include <cstdlib>

enum { QUERY_FWD = 0, QUERY_FWD_TRAIN = 1, QUERY_BWD_POINTS = 2, QUERY_SURFACE_STEP = 3, QUERY_BWD_TRAIN = 4 };      // the operation
enum { QUERY_K_SPLIT = 0, QUERY_K_FWD4 = 1, QUERY_K_FWD8 = 2, QUERY_K_BWD = 3 };   // query_fwd_x3_split / _fwd_f32 / _fwd_f32_w8 / _bwd_f32 _kernel
// the A/B switches, read ONCE per process: the sort, the kernel choice and the children the tests start all see one value
enum { QUERY_SW_W4 = 1, QUERY_SW_NOSPLIT = 2, QUERY_SW_NO_ONE_HEAD = 4 };
inline int query_switches() {
    // W4: the four-wave kernel where the eight-wave one is the default -- the fp32-MFMA heads' large inference queries (forward and
    // backward) and the training forward; NOSPLIT: the one-wave-per-head forward kernels for the fp16 x 3 heads; NO_ONE_HEAD: below
    static const int v = (getenv("CHORE_QUERY_W4") ? QUERY_SW_W4 : 0) | (getenv("CHORE_QUERY_X3_NOSPLIT") ? QUERY_SW_NOSPLIT : 0) |
                         (getenv("CHORE_QUERY_NO_ONE_HEAD") ? QUERY_SW_NO_ONE_HEAD : 0);
    return v;
}

struct QueryPlan {
    int family;                 // QUERY_K_*
    int dtype;                  // the maps' type (CHORE_F32 / CHORE_BF16 / CHORE_F16): the kernel's T
    int ncb = 2, waves = 4;     // the template's NCB (the eight-wave kernels: 1) and the waves of a workgroup
    bool train = false, staged = false, x3 = false, surf = false, one = false;      // the template flags
    int one_head = 0;           // ONE without SURF: the head that has the gradient (QueryArgs::one_head)
    int pts, threads;           // points per tile, threads per workgroup
    bool sort = false;          // launch_query_sort first: the forward runs in sorted order
};

// 64-point tiles unless they would leave CUs without a workgroup
inline bool query_small_tiles(int B, int N) { return (size_t)B * ((N + 63) / 64) <= 256; }

// fp16 x 3 backward, a few rounds of workgroups: a round of 64-point tiles takes 82 us, one of 32-point tiles 46 us (measured,
// one workgroup per CU either way), so e.g. 20 000 points (313 tiles = 2 rounds, the second a fifth full) finish sooner as
// 625 small tiles (3 rounds): 165 -> 137 us; from ~10 rounds on the 64-point tiles win on every count
inline bool x3_bwd_prefers_small(int B, int N) {
    const long long t64 = (long long)B * ((N + 63) / 64), t32 = (long long)B * ((N + 31) / 32);
    const long long r64 = (t64 + 255) / 256, r32 = (t32 + 255) / 256;
    return r32 * 455 < r64 * 825;
}
inline bool query_sort_covers(int N, int FH, int FW) { return ((FW + 7) / 8) * ((FH + 7) / 8) <= 256 && N >= 64; }

// the text with which the entry point refuses the combination (after "<entry point>: "), or nullptr.  dtype: the maps' type
// AFTER the heads flag is stripped -- CHORE_F16 | CHORE_HEADS_X3 must not get past: the training kernels read fp32 or bf16
inline const char* query_plan_refuses(int op, int dtype, bool x3, bool have_forward) {
    if ((op == QUERY_FWD_TRAIN || op == QUERY_BWD_TRAIN) && dtype != 0 /*CHORE_F32*/ && dtype != 1 /*CHORE_BF16*/)
        return "maps must be CHORE_F32 or CHORE_BF16 (fp16 maps are an inference mode)";
    if (op == QUERY_BWD_TRAIN && x3 && !have_forward) return "the fp16 x 3 heads need the staged forward";
    if (op == QUERY_SURFACE_STEP && !x3) return "needs the fp16 x 3 heads (CHORE_F16X3, or CHORE_HEADS_X3 with the maps' type)";
    return nullptr;
}

// live_mask: bit i = head i (df, parts, pca, centers) has an upstream gradient (backward to the points)
inline QueryPlan query_plan(int op, int dtype, bool x3, int B, int N, int FH, int FW, int live_mask, bool has_workspace,
                            bool have_forward, int switches) {
    QueryPlan p;
    p.dtype = dtype; p.x3 = x3; p.family = QUERY_K_BWD;
    const bool small = query_small_tiles(B, N), w4 = switches & QUERY_SW_W4, one_live = live_mask && !(live_mask & (live_mask - 1));
    auto eight = [&](int family) { p.family = family; p.waves = 8; p.ncb = 1; };
    switch (op) {
    case QUERY_FWD:
        p.family = QUERY_K_FWD4;
        if (x3 && !(switches & QUERY_SW_NOSPLIT)) {     // two waves per head, 32 * NCB points
            p.family = QUERY_K_SPLIT; p.waves = 8; p.ncb = small ? 1 : 2;
            // sorted order: asked for by passing a workspace; large queries on the split kernel (the only one that reads QueryArgs::perm)
            p.sort = has_workspace && N >= 8192 && query_sort_covers(N, FH, FW);
        } else if (small) p.ncb = 1;
        // (a single output asked for, CHORE.query_df: 32-point tiles do not pay -- a workgroup is placed with the registers of all
        // four waves, so the CU holds one whatever the three leaving waves free: 363 against 335 us at 8 x 20 000 points)
        // fp16 x 3: a k-step of MFMAs is 2.7 x shorter than the fp32 one for the same weight bytes, and the eight-wave kernel
        // (both waves of a head fetch the head's fragments) is bound by the L1's 64 B / clk: 0.227 ms against 0.203 ms for
        // four waves with two column blocks each (4 x 20 000 points; the eight-wave fp16 x 3 inference kernel was removed in round 8)
        else if (!x3 && !w4) eight(QUERY_K_FWD8);
        break;
    case QUERY_FWD_TRAIN:
        p.train = true; p.family = QUERY_K_FWD4;
        if (!w4) eight(QUERY_K_FWD8);
        break;
    case QUERY_BWD_POINTS:
    case QUERY_SURFACE_STEP:
        p.surf = op == QUERY_SURFACE_STEP;
        // one upstream gradient (the surface step's distance head, the generator's steps, most fit phases): the head's chain on two
        // waves of a 64-point tile wherever 64-point tiles fill the CUs (the 32-point rule below was measured on the one-wave chain)
        if (x3 && (p.surf || one_live) && !(switches & QUERY_SW_NO_ONE_HEAD) && !small) {
            p.one = true;
            for (int i = 0; i < 4 && !p.surf; ++i) if (live_mask >> i & 1) p.one_head = i;
        } else if (small || (x3 && x3_bwd_prefers_small(B, N))) p.ncb = 1;
        // fp16 x 3: four waves with two column blocks each, like the forward (the eight-wave kernel fetches every weight
        // fragment twice and is bound by the L1: 0.65 against 0.58 ms at 4 x 20 000 points)
        else if (!x3 && !w4) eight(QUERY_K_BWD);
        break;
    case QUERY_BWD_TRAIN:
        p.train = true; p.staged = have_forward;
        // the recompute and the staged fp32 variants are bound by their staging stores: measured slower with eight waves (39.4 vs
        // 38.6 ms per step); staged fp16 x 3: no recompute, the eight-wave kernel fits its registers
        // (an eight-wave fp16 x 3 RECOMPUTE kernel existed behind a switch through round 3: slower, and in round 2 it produced a
        // non-finite gradient about once in six runs of the graph-replayed fit that was never reproduced afterwards; removed in round 4)
        if (p.staged && x3) eight(QUERY_K_BWD);
        break;
    }
    // the split kernel's eight waves share the tile's 32 * NCB points; elsewhere every group of four waves has 32 * NCB of its own
    p.pts = p.family == QUERY_K_SPLIT ? 32 * p.ncb : 32 * p.ncb * (p.waves / 4);
    p.threads = 64 * p.waves;
    return p;
}
