// ordinal_depth.hip -- PHOSA's ordinal depth term for the object fit: the two input masks say who is in front.
//
// Where the image shows the person, the person is in front of anything else that projects there; where it shows the object,
// the object is.  The term punishes the pixels of the silhouette grid whose two depths contradict that: d_o, the depth of the
// object face that wins the pixel in chore_silhouette_fwd, against d_h, the depth of the body there, a constant buffer of the
// call.  It rides on the winner map the mask term computes anyway: no second rasterisation, no colour renderer.
//   chore_sil_depth           winner map -> depth image (zp of raster_weights at the winner, far_z where there is none): fills the
//                             occluder buffer once per call; its per-pixel function od_winner_depth is where the step's d_o
//                             comes from as well
//   chore_ordinal_depth_fwd   per pixel the case, the term log1p(exp(min(difference, c))) and its derivative `coef`; per frame the
//                             sum (a fixed tree) and four integer counts
//   chore_ordinal_depth_bwd   coef x upstream gradient through the depth rule of chore_render_bwd (raster_depth_bwd_sample /
//                             _face of raster_common.h), gathered per face like there: one workgroup per face, fixed order
// A pixel needs its winner's pixel-space inverse; the workspace is sized by (B, S) alone, so the pixel rebuilds it from the
// three vertices with tri_setup -- the expressions of the rasterisers' setup kernel, hence the same bits.  No float atomics,
// fills are stores of the kernels themselves, nothing is read on the host: the calls can be recorded into a graph.
#include "raster_common.h"

namespace {

constexpr int OD_TILE = 256;          // pixels (= threads) per block of the forward and of chore_sil_depth
constexpr int OD_MAX_DIM = 4096;      // chore_silhouette_fwd's limit

// depth of face `f9` (x y z x y z x y z) at pixel (x, y), rows not flipped, of an S x S grid: zp of raster_weights under the
// inverse tri_setup gives.  The single place a winner's depth is computed in this file.
__device__ __forceinline__ float od_winner_depth(const float* __restrict__ f9, int S, int x, int y) {
    TriSetup t;
#pragma unroll
    for (int k = 0; k < 9; ++k) t.f[k] = f9[k];
    tri_setup(t, S);
    float w[3], zp;
    raster_weights(t.f, t.inv, (float)x, (float)y, w, zp);
    return zp;
}

// thread = pixel (x fastest) of the winner map; the output row is S - 1 - y with `flip`
__global__ __launch_bounds__(OD_TILE) void od_depth_kernel(const float* __restrict__ tri, const int* __restrict__ fim, int F, int S,
                                                          float far, int flip, float* __restrict__ depth) {
    const int p = blockIdx.x * OD_TILE + threadIdx.x;
    if (p >= S * S) return;
    const int b = blockIdx.y, y = p / S, x = p - y * S;
    const size_t img = (size_t)b * S * S;
    const int fn = fim[img + p];
    float d = far;
    if (fn >= 0 && fn < F) d = od_winner_depth(tri + ((size_t)b * F + fn) * 9, S, x, y);
    depth[img + (size_t)(flip ? S - 1 - y : y) * S + x] = d;
}

// thread = pixel (r, x) of the masks' orientation, i.e. row S - 1 - r of the winner map.  A tree over the block's OD_TILE
// terms (8 levels), one partial sum and four partial counts per block.
__global__ __launch_bounds__(OD_TILE) void od_fwd_kernel(const float* __restrict__ tri, const int* __restrict__ fim,
                                                        const float* __restrict__ occ, const float* __restrict__ image_ref,
                                                        const float* __restrict__ keep_mask, int F, int S, float far, float c,
                                                        float* __restrict__ coef, float* __restrict__ partial,
                                                        int* __restrict__ cpartial) {
    __shared__ float s[OD_TILE];
    __shared__ int cnt[4][4];
    const int p = blockIdx.x * OD_TILE + threadIdx.x;
    const int b = blockIdx.y;
    const size_t img = (size_t)b * S * S;
    float term = 0.f;
    bool in_a = false, in_b = false, pb = false, ob = false;
    if (p < S * S) {
        const int r = p / S, x = p - r * S, y = S - 1 - r;
        const int fn = fim[img + (size_t)y * S + x];
        const float dh = occ[img + p];
        const bool both = fn >= 0 && fn < F && dh < far;
        const bool O = image_ref[img + p] > 0.5f;           // a pixel labelled both ways counts as object (cvt_masks)
        const bool P = !O && keep_mask[img + p] < 0.5f;
        float cf = 0.f;
        if (both && (P || O)) {
            pb = P; ob = O;
            const float d_o = od_winner_depth(tri + ((size_t)b * F + fn) * 9, S, x, y);
            const float diff = P ? __fsub_rn(dh, d_o) : __fsub_rn(d_o, dh);      // > 0: the ordering the mask states is violated
            if (diff > 0.f) {
                in_a = P; in_b = O;
                const float xv = fminf(diff, c);
                term = log1pf(expf(xv));
                if (diff <= c) {                           // the clamp passes the gradient at equality, like torch.clamp
                    const float sg = 1.0f / (1.0f + expf(-xv));
                    cf = P ? -sg : sg;
                }
            }
        }
        coef[img + p] = cf;
    }
    const int wv = threadIdx.x >> 6;
    const unsigned long long ma = __ballot(in_a), mb = __ballot(in_b), mp = __ballot(pb), mo = __ballot(ob);
    if ((threadIdx.x & 63) == 0) {
        cnt[wv][0] = __popcll(ma); cnt[wv][1] = __popcll(mb); cnt[wv][2] = __popcll(mp); cnt[wv][3] = __popcll(mo);
    }
    s[threadIdx.x] = term;
    __syncthreads();
    for (int k = OD_TILE / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
        __syncthreads();
    }
    const size_t blk = (size_t)b * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) partial[blk] = s[0];
    if (threadIdx.x < 4) cpartial[blk * 4 + threadIdx.x] = (cnt[0][threadIdx.x] + cnt[1][threadIdx.x]) + (cnt[2][threadIdx.x] + cnt[3][threadIdx.x]);
}

// the frame's partials: thread t adds partials t, t + OD_TILE, ... in order, then the same tree; the counts likewise (integers)
__global__ __launch_bounds__(OD_TILE) void od_sum_kernel(const float* __restrict__ partial, const int* __restrict__ cpartial, int nblk,
                                                        float* __restrict__ out, int* __restrict__ counts) {
    __shared__ float s[OD_TILE];
    __shared__ int ci[4][OD_TILE];
    const int b = blockIdx.x;
    float acc = 0.f;
    int ca[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < nblk; i += OD_TILE) {
        acc += partial[(size_t)b * nblk + i];
#pragma unroll
        for (int k = 0; k < 4; ++k) ca[k] += cpartial[((size_t)b * nblk + i) * 4 + k];
    }
    s[threadIdx.x] = acc;
#pragma unroll
    for (int k = 0; k < 4; ++k) ci[k][threadIdx.x] = ca[k];
    __syncthreads();
    for (int k = OD_TILE / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) {
            s[threadIdx.x] += s[threadIdx.x + k];
#pragma unroll
            for (int q = 0; q < 4; ++q) ci[q][threadIdx.x] += ci[q][threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[b] = s[0];
    if (threadIdx.x < 4) counts[b * 4 + threadIdx.x] = ci[threadIdx.x][0];
}

// One workgroup per face, as render_bwd.hip's gather and with its walk (raster_for_each_won_pixel: the aligned 16 x 16 tiles the
// box meets, the pixels the face won, their weights and depth rebuilt): coef x g summed per thread in tile order, then over the
// workgroup by raster_wg_sum's fixed tree.  Every face is written: zeros for one that won no pixel.
__global__ __launch_bounds__(256) void od_bwd_kernel(const float* __restrict__ tri, const int* __restrict__ fim,
                                                    const float* __restrict__ coef, const float* __restrict__ g, int F, int S,
                                                    float* __restrict__ grad_tri) {
    __shared__ float red[4][3];
    __shared__ TriSetup tsh;
    const int i = blockIdx.x;
    const int b = i / F, fn = i - b * F;
    const int tid = threadIdx.x;
    if (tid == 0) {
        TriSetup t0;
#pragma unroll
        for (int k = 0; k < 9; ++k) t0.f[k] = tri[(size_t)i * 9 + k];
        tri_setup(t0, S);
        tsh = t0;
    }
    __syncthreads();
    const TriSetup& t = tsh;
    float* out = grad_tri + (size_t)i * 9;
    if (t.x0 > t.x1 || t.y0 > t.y1) {                    // culled or out of view: it won no pixel
        if (tid < 9) out[tid] = 0.f;
        return;
    }
    const size_t img = (size_t)b * S * S;
    const float gb = g[b];
    float acc[3] = {0.f, 0.f, 0.f};
    const int mine = raster_for_each_won_pixel(t, fim + img, fn, S, [&](size_t, int x, int y, const float* w, float zp) {
        raster_depth_bwd_sample(__fmul_rn(coef[img + (size_t)(S - 1 - y) * S + x], gb), w, zp, acc);
    });
    if (!__syncthreads_or(mine)) {
        if (tid < 9) out[tid] = 0.f;
        return;
    }
    raster_wg_sum<3>(acc, red);
    if (tid == 0) {
        float g9[9];
        raster_depth_bwd_face(t, red[0], S, g9);
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = g9[k];
    }
}

bool od_sizes_ok(int B, int F, int S) {
    return B > 0 && B <= 65535 && F > 0 && S > 0 && S <= OD_MAX_DIM && (long long)B * F <= 0x7fffffffLL / 32;
}
int od_blocks(int S) { return (S * S + OD_TILE - 1) / OD_TILE; }

// workspace of chore_ordinal_depth_fwd: one float per block of the forward | four ints per block
struct OrdinalDepthWs { float* partial; int* cpartial; size_t bytes; };
OrdinalDepthWs ordinal_depth_ws(void* base, int B, int S) {
    const size_t n = (size_t)B * od_blocks(S);
    WsCarver c(base);
    return {c.take<float>(n), c.take<int>(4 * n), c.bytes};
}

}  // namespace

extern "C" int chore_sil_depth(chore_handle* h, const float* tri, const int* face_index, int B, int F, int S, float far_z,
                               int flip_rows, float* depth, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!tri || !face_index || !depth) CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_depth: null argument");
    if (!od_sizes_ok(B, F, S)) CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_depth: bad sizes B=%d F=%d S=%d", B, F, S);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(od_depth_kernel, dim3(od_blocks(S), B), dim3(OD_TILE), 0, s, tri, face_index, F, S, far_z, flip_rows ? 1 : 0, depth);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" size_t chore_ordinal_depth_workspace_bytes(int B, int S) {
    return od_sizes_ok(B, 1, S) ? ordinal_depth_ws(nullptr, B, S).bytes : 0;
}

extern "C" int chore_ordinal_depth_fwd(chore_handle* h, const float* tri, const int* face_index, const float* occluder_depth,
                                       const float* image_ref, const float* keep_mask, int B, int F, int S, float far_z, float c,
                                       float* per_frame_sum, float* coef, int* counts, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!tri || !face_index || !occluder_depth || !image_ref || !keep_mask || !per_frame_sum || !coef || !counts || !workspace)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_ordinal_depth_fwd: null argument");
    if (!od_sizes_ok(B, F, S) || !(c > 0.f) || !(c <= 80.f))      // exp(c) stays finite in float
        CHORE_FAIL(h, CHORE_EINVAL, "chore_ordinal_depth_fwd: bad sizes B=%d F=%d S=%d c=%g", B, F, S, (double)c);
    hipStream_t s = (hipStream_t)stream;
    const OrdinalDepthWs w = ordinal_depth_ws(workspace, B, S);
    const int nblk = od_blocks(S);
    hipLaunchKernelGGL(od_fwd_kernel, dim3(nblk, B), dim3(OD_TILE), 0, s, tri, face_index, occluder_depth, image_ref, keep_mask, F, S,
                       far_z, c, coef, w.partial, w.cpartial);
    hipLaunchKernelGGL(od_sum_kernel, dim3(B), dim3(OD_TILE), 0, s, (const float*)w.partial, (const int*)w.cpartial, nblk,
                       per_frame_sum, counts);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" int chore_ordinal_depth_bwd(chore_handle* h, const float* tri, const int* face_index, const float* coef,
                                       const float* g_per_frame, int B, int F, int S, float* grad_tri, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!tri || !face_index || !coef || !g_per_frame || !grad_tri) CHORE_FAIL(h, CHORE_EINVAL, "chore_ordinal_depth_bwd: null argument");
    if (!od_sizes_ok(B, F, S)) CHORE_FAIL(h, CHORE_EINVAL, "chore_ordinal_depth_bwd: bad sizes B=%d F=%d S=%d", B, F, S);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(od_bwd_kernel, dim3(B * F), dim3(256), 0, s, tri, face_index, coef, g_per_frame, F, S, grad_tri);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
