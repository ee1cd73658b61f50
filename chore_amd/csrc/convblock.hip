// convblock.hip -- one ConvBlock of the stacked hourglass as a TRAINING operator: forward and backward in one call each.
//
// ConvBlock (/root/reference/model/net_util.py:346-396), 43 of them per encoder pass:
//     o1 = conv3x3(relu(gn1(x)))   Cin    -> Cout/2
//     o2 = conv3x3(relu(gn2(o1)))  Cout/2 -> Cout/4
//     o3 = conv3x3(relu(gn3(o2)))  Cout/4 -> Cout/4
//     y  = cat(o1, o2, o3) + (x  or  conv1x1(relu(gn4(x))) when Cin != Cout)
// Composing this from per-layer autograd nodes (ops.hip) costs a concat, a residual add, strided-slice copies and
// gradient sums around every block, all of them elementwise passes over HBM and host work.  Here the block is laid out the
// way the inference program lays it out (encoder.hip, conv_block): every convolution writes its slice of y with the residual
// added in its epilogue, the raw o1 / o2 go to their own buffers, and the GroupNorm statistics of o1, o2 and y come from
// the same epilogues.  The backward reads dy in channel-strided slices (wgrad / dgrad take a row stride) and the
// GroupNorm backward adds the skip gradients on its way out, so no glue kernel runs at all.
// The arithmetic of every kernel is unchanged; in fp32 the results equal the per-layer composition bit for bit.
#include "enc_common.h"
#include <cstdlib>

namespace {

struct Dims {
    int B, H, W, Cin, Cout, C1, C2;
    size_t px, es, nb;       // pixels, element size, bytes of one statistics block
    bool down;
};

bool make_dims(Dims& d, int dtype, int B, int H, int W, int Cin, int Cout) {
    if ((dtype != CHORE_F32 && dtype != CHORE_BF16 && dtype != CHORE_F16X3) || B <= 0 || H <= 0 || W <= 0) return false;
    if (Cout % 128 || Cin % 32 || Cin > 256 || Cout > 256) return false;      // slices of Cout/4 channels, whole groups
    d.B = B; d.H = H; d.W = W; d.Cin = Cin; d.Cout = Cout; d.C1 = Cout / 2; d.C2 = Cout / 4;
    d.px = (size_t)B * H * W; d.es = dtype == CHORE_BF16 ? 2 : 4; d.nb = act_stats_bytes(B);
    d.down = Cin != Cout;
    return true;
}
// What the block's launches accept of a shape make_dims lets through: every GroupNorm(32, C) of the block -- over Cin (bn1, bn4),
// Cout/2, Cout/4 and the statistics of y over Cout -- needs a group size of 1, 2, 4 or 8.  Cout in {128, 256} always has one;
// Cin = 96, 160, 192, 224 has not.  Both entry points ask BEFORE their first launch: the launches refuse such a Cin themselves,
// but in the backward only the last GroupNorm backward does, after weight-gradient kernels went onto the side stream -- the call
// then returned without the join, with kernels still writing the caller's workspace.  (The size functions keep answering
// for every shape make_dims accepts.)  -> the offending channel count, 0: fine
int bad_group_channels(const Dims& d) {
    for (int c : {d.Cin, d.Cout, d.C1, d.C2})
        if (!conv_gn_group_ok(c)) return c;
    return 0;
}

// saved (forward -> backward): statistics [x | o1 | o2 | y], then o1, o2
struct Saved {
    char *sx, *s1, *s2, *sy, *o1, *o2;
    size_t bytes;
};
Saved saved_layout(const Dims& d, void* base) {
    WsCarver c(base);
    return {c.raw<char>(d.nb), c.raw<char>(d.nb), c.raw<char>(d.nb), c.take<char>(d.nb),
            c.take<char>(d.px * d.C1 * d.es), c.take<char>(d.px * d.C2 * d.es), c.bytes};
}

// the block's packed weights: the whole forward workspace, a part of the backward's (the transposed, data-gradient forms have
// the same sizes).  wd: with d.down only
struct Packed { char *w1, *w2, *w3, *wd; };
Packed pack_layout(const Dims& d, int dtype, WsCarver& c) {
    return {c.take<char>(packed_conv_bytes(dtype, 9, d.Cin, d.C1)), c.take<char>(packed_conv_bytes(dtype, 9, d.C1, d.C2)),
            c.take<char>(packed_conv_bytes(dtype, 9, d.C2, d.C2)), c.take<char>(d.down ? packed_conv_bytes(dtype, 1, d.Cin, d.Cout) : 0)};
}

// the handle's side stream and its events (lazily created on the handle's device)
int side_stream(chore_handle* h) {
    if (h->side) return CHORE_OK;
    CHORE_HIP_CHECK(h, hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    for (hipEvent_t& e : h->side_ev) CHORE_HIP_CHECK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return CHORE_OK;
}

View mkview(const void* p, int cs, int co, int C) { View v; v.p = const_cast<void*>(p); v.cs = cs; v.co = co; v.C = C; return v; }

size_t gn_acc_bytes(int B, int C) { return chore_gn_relu_bwd_workspace_bytes(B, C); }   // two tables of cells (enc_common.h)

// backward workspace: GroupNorm-backward accumulators, range cells of d(o2), d(o1): the first zero_bytes, cleared by the pack
// launch | range cells of dy | transposed packed weights | wgrad partials | da | d(o2) | d(o1) | dx4.  Range cells (fp16 x 3):
// every gradient tensor that feeds a GEMM carries max |g| (enc_common.h, AMAX_CELLS): of dy from a reduction that rides in
// the pack launch, of d(o2) / d(o1) from the GroupNorm backward that writes them
struct BwdWs {
    char *acc1, *acc4, *acc2, *acc3;
    unsigned *amax_o2, *amax_o1, *amax_dy;
    size_t zero_bytes;
    Packed pk;
    char *wpart1, *wpart2, *wpart3, *wpartd, *da, *do2, *do1, *dx4;
    size_t bytes;
};
BwdWs bwd_layout(const Dims& d, int dtype, void* base) {
    const int B = d.B, H = d.H, W = d.W, Cin = d.Cin, C1 = d.C1, C2 = d.C2;
    WsCarver c(base);
    BwdWs w;
    w.acc1 = c.raw<char>(gn_acc_bytes(B, Cin)); w.acc4 = c.raw<char>(gn_acc_bytes(B, Cin));
    w.acc2 = c.raw<char>(gn_acc_bytes(B, C1)); w.acc3 = c.raw<char>(gn_acc_bytes(B, C2));
    w.amax_o2 = c.raw<unsigned>(AMAX_CELLS); w.amax_o1 = c.take<unsigned>(AMAX_CELLS);
    w.zero_bytes = c.bytes;
    w.amax_dy = c.raw<unsigned>(AMAX_CELLS);      // plain stores: outside the cleared region
    w.pk = pack_layout(d, dtype, c);
    // the four weight gradients keep their shares' partials until ONE launch sums all of them: a region each
    w.wpart1 = c.take<char>(chore_conv2d_wgrad_workspace_bytes(9, B, H, W, Cin, C1));
    w.wpart2 = c.take<char>(chore_conv2d_wgrad_workspace_bytes(9, B, H, W, C1, C2));
    w.wpart3 = c.take<char>(chore_conv2d_wgrad_workspace_bytes(9, B, H, W, C2, C2));
    w.wpartd = c.take<char>(d.down ? chore_conv2d_wgrad_workspace_bytes(1, B, H, W, Cin, d.Cout) : 0);
    w.da = c.take<char>(d.px * (size_t)(Cin > C1 ? Cin : C1) * d.es);
    w.do2 = c.take<char>(d.px * C2 * d.es);
    w.do1 = c.take<char>(d.px * C1 * d.es);
    w.dx4 = c.take<char>(d.down ? d.px * Cin * d.es : 0);      // gradient through the downsample branch
    w.bytes = c.bytes;
    return w;
}

}  // namespace

extern "C" {

size_t chore_convblock_saved_bytes(int dtype, int B, int H, int W, int Cin, int Cout) {
    Dims d;
    if (!make_dims(d, dtype, B, H, W, Cin, Cout)) return 0;
    return saved_layout(d, nullptr).bytes;
}
// byte offset of the statistics of y inside `saved` (chore_gn_stats_bytes(B) of them): what the NEXT block's x_stats wants
size_t chore_convblock_out_stats_offset(int B) { return 3 * act_stats_bytes(B); }

size_t chore_convblock_workspace_bytes(int dtype, int B, int H, int W, int Cin, int Cout) {
    Dims d;
    if (!make_dims(d, dtype, B, H, W, Cin, Cout)) return 0;
    WsCarver fwd(nullptr);
    pack_layout(d, dtype, fwd);
    const size_t bwd = bwd_layout(d, dtype, nullptr).bytes;
    return fwd.bytes > bwd ? fwd.bytes : bwd;
}
// floats of the parameter-gradient arena: dW1 dW2 dW3 [dWd] then (dgamma, dbeta) of bn1, bn2, bn3 [, bn4]
size_t chore_convblock_grad_floats(int Cin, int Cout) {
    const size_t C1 = Cout / 2, C2 = Cout / 4;
    size_t n = 9 * ((size_t)Cin * C1 + C1 * C2 + C2 * C2) + 2 * (Cin + C1 + C2);
    if (Cin != Cout) n += (size_t)Cin * Cout + 2 * Cin;
    return n;
}

// y (B,H,W,Cout) = ConvBlock(x (B,H,W,Cin)).  Weights: reference layout fp32, no biases (conv3x3(bias=False));
// wd / g4 / b4 only when Cin != Cout.  x_stats: GroupNorm statistics of x (e.g. the previous block's, see
// chore_convblock_out_stats_offset) or NULL: computed here.  saved: chore_convblock_saved_bytes, kept for the backward.
int chore_convblock_fwd(chore_handle* h, int dtype, const void* x, const void* x_stats, int B, int H, int W, int Cin, int Cout,
                        const float* w1, const float* w2, const float* w3, const float* wd, const float* const* gb /*[8]: g1 b1 g2 b2 g3 b3 g4 b4*/,
                        void* y, void* saved, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    Dims d;
    if (!make_dims(d, dtype, B, H, W, Cin, Cout)) CHORE_FAIL(h, CHORE_EINVAL, "chore_convblock_fwd: unsupported shape Cin=%d Cout=%d", Cin, Cout);
    if (const int c = bad_group_channels(d))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_convblock_fwd: GroupNorm over %d channels unsupported (group size must be 1, 2, 4 or 8; Cin=%d Cout=%d)", c, Cin, Cout);
    if (d.down && !wd) CHORE_FAIL(h, CHORE_EINVAL, "chore_convblock_fwd: Cin=%d != Cout=%d needs the downsample weight wd", Cin, Cout);
    if (!x || !w1 || !w2 || !w3 || !gb || !y || !saved || !workspace || (d.down && !wd))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_convblock_fwd: null argument");
    hipStream_t s = (hipStream_t)stream;
    const Saved sv = saved_layout(d, saved);
    WsCarver c(workspace);
    const Packed pk = pack_layout(d, dtype, c);
    int rc;
    {   // one launch: the block's weights in fragment order, the statistics accumulators cleared
        PackJobs pj;
        pj.add(w1, pk.w1, 9, Cin, d.C1, 0);
        pj.add(w2, pk.w2, 9, d.C1, d.C2, 0);
        pj.add(w3, pk.w3, 9, d.C2, d.C2, 0);
        if (d.down) pj.add(wd, pk.wd, 1, Cin, Cout, 0);
        pj.zero = sv.sx; pj.zero_vecs = 4 * d.nb / 16;
        if ((rc = launch_pack_conv_multi(h, dtype, pj, s))) return rc;
    }
    const GroupStat* sx = (const GroupStat*)x_stats;
    if (!sx) {
        if ((rc = launch_gn_stats(h, dtype == CHORE_F16X3 ? CHORE_F32 : dtype, mkview(x, Cin, 0, Cin), B, H * W, (GroupStat*)sv.sx, s))) return rc;
        sx = (const GroupStat*)sv.sx;
    }
    const void* res = x;
    int res_cs = Cin;
    if (d.down) {      // residual = conv1x1(relu(gn4(x))), written to y and picked up from there
        ConvArgs a{};
        a.in = mkview(x, Cin, 0, Cin); a.in_st = sx; a.gamma = gb[6]; a.beta = gb[7];
        a.wpk = pk.wd;
        a.out = mkview(y, Cout, 0, Cout);
        a.B = B; a.H = H; a.W = W; a.Cout = Cout;
        if ((rc = launch_conv(h, dtype, 1, a, s))) return rc;
        res = y; res_cs = Cout;
    }
    {   // conv1
        ConvArgs a{};
        a.in = mkview(x, Cin, 0, Cin); a.in_st = sx; a.gamma = gb[0]; a.beta = gb[1];
        a.wpk = pk.w1;
        a.out = mkview(y, Cout, 0, d.C1); a.raw = mkview(sv.o1, d.C1, 0, d.C1); a.res = mkview(res, res_cs, 0, d.C1);
        a.B = B; a.H = H; a.W = W; a.Cout = d.C1;
        a.st_raw = (GroupStat*)sv.s1; a.st_raw_C = d.C1; a.st_raw_co = 0;
        a.st_out = (GroupStat*)sv.sy; a.st_out_C = Cout; a.st_out_co = 0;
        if ((rc = launch_conv(h, dtype, 9, a, s))) return rc;
    }
    {   // conv2
        ConvArgs a{};
        a.in = mkview(sv.o1, d.C1, 0, d.C1); a.in_st = (const GroupStat*)sv.s1; a.gamma = gb[2]; a.beta = gb[3];
        a.wpk = pk.w2;
        a.out = mkview(y, Cout, d.C1, d.C2); a.raw = mkview(sv.o2, d.C2, 0, d.C2); a.res = mkview(res, res_cs, d.C1, d.C2);
        a.B = B; a.H = H; a.W = W; a.Cout = d.C2;
        a.st_raw = (GroupStat*)sv.s2; a.st_raw_C = d.C2; a.st_raw_co = 0;
        a.st_out = (GroupStat*)sv.sy; a.st_out_C = Cout; a.st_out_co = d.C1;
        if ((rc = launch_conv(h, dtype, 9, a, s))) return rc;
    }
    {   // conv3
        ConvArgs a{};
        a.in = mkview(sv.o2, d.C2, 0, d.C2); a.in_st = (const GroupStat*)sv.s2; a.gamma = gb[4]; a.beta = gb[5];
        a.wpk = pk.w3;
        a.out = mkview(y, Cout, d.C1 + d.C2, d.C2); a.res = mkview(res, res_cs, d.C1 + d.C2, d.C2);
        a.B = B; a.H = H; a.W = W; a.Cout = d.C2;
        a.st_out = (GroupStat*)sv.sy; a.st_out_C = Cout; a.st_out_co = d.C1 + d.C2;
        if ((rc = launch_conv(h, dtype, 9, a, s))) return rc;
    }
    return CHORE_OK;
}

// dx (B,H,W,Cin) and the parameter gradients (chore_convblock_grad_floats, layout there) from dy (B,H,W,Cout, dense).
// x_stats: what the forward used (NULL: the ones it computed, in `saved`).
int chore_convblock_bwd(chore_handle* h, int dtype, const void* x, const void* x_stats, const void* dy, int B, int H, int W, int Cin,
                        int Cout, const float* w1, const float* w2, const float* w3, const float* wd, const float* const* gb,
                        const void* saved, void* dx, float* grads, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    Dims d;
    if (!make_dims(d, dtype, B, H, W, Cin, Cout)) CHORE_FAIL(h, CHORE_EINVAL, "chore_convblock_bwd: unsupported shape Cin=%d Cout=%d", Cin, Cout);
    if (const int c = bad_group_channels(d))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_convblock_bwd: GroupNorm over %d channels unsupported (group size must be 1, 2, 4 or 8; Cin=%d Cout=%d)", c, Cin, Cout);
    if (d.down && !wd) CHORE_FAIL(h, CHORE_EINVAL, "chore_convblock_bwd: Cin=%d != Cout=%d needs the downsample weight wd", Cin, Cout);
    if (!x || !dy || !w1 || !w2 || !w3 || !gb || !saved || !dx || !grads || !workspace || (d.down && !wd))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_convblock_bwd: null argument");
    hipStream_t s = (hipStream_t)stream;
    const Saved sv = saved_layout(d, const_cast<void*>(saved));
    const void* sx = x_stats ? x_stats : (const void*)sv.sx;
    const int C1 = d.C1, C2 = d.C2, HW = H * W;
    const BwdWs bw = bwd_layout(d, dtype, workspace);
    const bool x3 = dtype == CHORE_F16X3;
    WgradFinishJobs fin;            // the four ordered sums over the shares: one launch at the end of the side chain
    // gradient arena
    float* dw1 = grads; float* dw2 = dw1 + (size_t)9 * Cin * C1; float* dw3 = dw2 + (size_t)9 * C1 * C2;
    float* dwd = dw3 + (size_t)9 * C2 * C2;
    float* gbp = dwd + (d.down ? (size_t)Cin * Cout : 0);
    float *dg1 = gbp, *db1 = dg1 + Cin, *dg2 = db1 + Cin, *db2 = dg2 + C1, *dg3 = db2 + C1, *db3 = dg3 + C2, *dg4 = db3 + C2, *db4 = dg4 + Cin;
    const char* dyb = (const char*)dy;
    int rc;
    {   // one launch: the transposed, flipped weights of the data-gradient convolutions; the accumulators cleared
        PackJobs pj;
        pj.add(w1, bw.pk.w1, 9, C1, Cin, 1);
        pj.add(w2, bw.pk.w2, 9, C2, C1, 1);
        pj.add(w3, bw.pk.w3, 9, C2, C2, 1);
        if (d.down) pj.add(wd, bw.pk.wd, 1, Cout, Cin, 1);
        pj.zero = workspace; pj.zero_vecs = bw.zero_bytes / 16;
        if (x3) { pj.amax_x = (const float*)dy; pj.amax_n4 = d.px * (size_t)Cout / 4; pj.amax_cells = bw.amax_dy; }
        if ((rc = launch_pack_conv_multi(h, dtype, pj, s))) return rc;
    }
    const int adt = x3 ? CHORE_F32 : dtype;          // the element type of the tensors (what the non-GEMM kernels see)
    (void)adt;
    auto dgrad = [&](int taps, const View& in, const float* w, const char* wpk, int cin_fwd, int cout_fwd, void* out, const unsigned* amax) -> int {
        // data gradient of a layer Cin_fwd -> Cout_fwd: the forward kernel on the transposed, flipped weights
        (void)w; (void)cout_fwd;
        ConvArgs a{};
        a.in = in;
        a.wpk = wpk;
        a.out = mkview(out, cin_fwd, 0, cin_fwd);
        a.B = B; a.H = H; a.W = W; a.Cout = cin_fwd;
        a.in_amax = x3 ? amax : nullptr;
        return launch_conv(h, dtype, taps, a, s);
    };
    // Two chains: the data-gradient chain  dgrad3 -> gn3 -> dgrad2 -> gn2 -> [downsample] -> dgrad1 -> gn1  on the
    // caller's stream, and the four weight gradients on the handle's side stream, each released by the event after the
    // kernel that produces its dy (dy itself for conv3 and the downsample conv).  The kernels of either chain fill a
    // fraction of the chip (64 .. 256 workgroups), so the chains overlap almost completely.
    static const bool serial = getenv("CHORE_CONVBLOCK_SERIAL") != nullptr;      // A/B switch: everything on one stream
    hipStream_t s2 = s;
    if (!serial) {
        if ((rc = side_stream(h))) return rc;
        s2 = h->side;
    }
    auto release = [&](int ev) -> int {      // side stream waits for what the main stream has issued so far
        if (serial) return CHORE_OK;
        CHORE_HIP_CHECK(h, hipEventRecord(h->side_ev[ev], s));
        CHORE_HIP_CHECK(h, hipStreamWaitEvent(s2, h->side_ev[ev], 0));
        return CHORE_OK;
    };
    const int off2 = C1, off3 = C1 + C2;
    // Launch order inside a stage: the data-gradient kernels (caller's stream) BEFORE the weight-gradient kernels (side stream)
    // that the same event releases.  Eagerly it makes no difference; recorded into a hipGraph it does: the runtime lays the
    // graph out on queues by following every node's FIRST-recorded successor, so with the side kernel recorded first the
    // data-gradient chain changed queue at each of the three releases, ~10 us per change (profiles/r04_train_graph.txt).
    if ((rc = release(0))) return rc;        // dy, the workspace clear
    // ---- conv3: its output gradient is the last slice of dy ----
    if ((rc = dgrad(9, mkview(dy, Cout, off3, C2), w3, bw.pk.w3, C2, C2, bw.da, bw.amax_dy))) return rc;
    if ((rc = gn_relu_bwd_impl(h, dtype, sv.o2, sv.s2, gb[4], gb[5], bw.da, B, HW, C2, bw.do2, dg3, db3, bw.acc3, 1,
                               dyb + (size_t)off2 * d.es, Cout, s, x3 ? bw.amax_o2 : nullptr))) return rc;          // + the concat's gradient of o2
    if ((rc = conv2d_bwd_weight_impl(h, dtype, 9, sv.o2, B, H, W, C2, sv.s2, gb[4], gb[5], dyb + (size_t)off3 * d.es, Cout, C2, dw3,
                                     nullptr, bw.wpart3, s2, &fin, x3 ? bw.amax_dy : nullptr))) return rc;
    if (d.down && (rc = conv2d_bwd_weight_impl(h, dtype, 1, x, B, H, W, Cin, sx, gb[6], gb[7], dy, Cout, Cout, dwd, nullptr, bw.wpartd, s2, &fin,
                                               x3 ? bw.amax_dy : nullptr)))
        return rc;
    // ---- conv2 ----
    if ((rc = release(1))) return rc;        // d(o2)
    if ((rc = dgrad(9, mkview(bw.do2, C2, 0, C2), w2, bw.pk.w2, C1, C2, bw.da, bw.amax_o2))) return rc;
    if ((rc = gn_relu_bwd_impl(h, dtype, sv.o1, sv.s1, gb[2], gb[3], bw.da, B, HW, C1, bw.do1, dg2, db2, bw.acc2, 1, dyb, Cout, s,
                               x3 ? bw.amax_o1 : nullptr))) return rc;
    if ((rc = conv2d_bwd_weight_impl(h, dtype, 9, sv.o1, B, H, W, C1, sv.s1, gb[2], gb[3], bw.do2, C2, C2, dw2, nullptr, bw.wpart2, s2, &fin,
                                     x3 ? bw.amax_o2 : nullptr))) return rc;
    // ---- conv1 (and the downsample branch): both normalise x ----
    if ((rc = release(2))) return rc;        // d(o1)
    const void* skip = dy;          // identity residual: dy itself flows to x
    int skip_cs = Cout;
    if (d.down) {
        if ((rc = dgrad(1, mkview(dy, Cout, 0, Cout), wd, bw.pk.wd, Cin, Cout, bw.da, bw.amax_dy))) return rc;
        if ((rc = gn_relu_bwd_impl(h, dtype, x, sx, gb[6], gb[7], bw.da, B, HW, Cin, bw.dx4, dg4, db4, bw.acc4, 1, nullptr, 0, s))) return rc;
        skip = bw.dx4; skip_cs = Cin;
    }
    if ((rc = dgrad(9, mkview(bw.do1, C1, 0, C1), w1, bw.pk.w1, Cin, C1, bw.da, bw.amax_o1))) return rc;
    if ((rc = gn_relu_bwd_impl(h, dtype, x, sx, gb[0], gb[1], bw.da, B, HW, Cin, dx, dg1, db1, bw.acc1, 1, skip, skip_cs, s))) return rc;
    if ((rc = conv2d_bwd_weight_impl(h, dtype, 9, x, B, H, W, Cin, sx, gb[0], gb[1], bw.do1, C1, C1, dw1, nullptr, bw.wpart1, s2, &fin,
                                     x3 ? bw.amax_o1 : nullptr))) return rc;
    if ((rc = launch_wgrad_finish_multi(h, fin, s2))) return rc;
    if (!serial) {                    // join: the caller's stream continues after the weight gradients too
        CHORE_HIP_CHECK(h, hipEventRecord(h->side_ev[3], s2));
        CHORE_HIP_CHECK(h, hipStreamWaitEvent(s, h->side_ev[3], 0));
    }
    return CHORE_OK;
}

}  // extern "C"
