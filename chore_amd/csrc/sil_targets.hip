// sil_targets.hip -- the silhouette term's targets, built on the device, and PHOSA's edge term.
//
// Replaces what SilLossROI's constructor does on the host (recon/obj_pose_roi.py:21-103,125-157: the object mask's box with
// np.nonzero, PHOSA's make_bbox_square, to_original_bbox, compute_K_roi, one grid_sample per frame and mask, cvt_masks,
// compute_edges and scipy.ndimage.distance_transform_edt per frame) with fixed-shape launches that read no device value on the
// host, so a fitting chain can refresh its targets inside a recorded graph:
//   chore_edt_sq        exact squared Euclidean distance transform, int32 (column pass, then a row pass through LDS)
//   chore_sil_edge_edt  edges = maxpool_k(image_ref) - image_ref and edt = (distance to the nearest edge pixel) ^ (2 power)
//   chore_sil_targets   box of obj > 0.5 (integer atomics) -> square box, ROI intrinsics (double, the host's operation order)
//                       -> bilinear crops of both masks (double), thresholds, cvt_masks
//   chore_sil_edge_fwd / _bwd   sum_pixels (maxpool_k(image) - image) * weight per frame and its gradient in gather form
// Fills are kernels (the launches are recorded into hipGraphs), atomics are integer only, every float sum has a fixed order:
// the same inputs give the same bits.
#include "common.h"
#include <limits.h>

namespace {

constexpr int EDT_MAX_DIM = 4096;        // d2 <= 2 * 4095^2 < 2^25; the row pass's LDS row is EDT_MAX_DIM ints (16 KB)
constexpr int EDT_COL_TILE = 64;         // columns per block of the column pass (one thread walks one column)
constexpr int EDT_ROW_TILE = 256;        // threads per block of the row pass (one block per row, pixels strided by this)
constexpr int EDT_INF = 1 << 30;         // "no feature in this column"; (x-x')^2 < 2^24 added to it stays below 2^31
constexpr int EDGE_TILE = 256;           // pixels (= threads) per block of the edge term's forward
constexpr int EDGE_MAX_K = 31;

// ---- exact squared distance transform ----------------------------------------------------------------------------------
// column pass: g2[b,y,x] = (distance to the nearest feature pixel of column x)^2, EDT_INF if the column has none
__global__ __launch_bounds__(EDT_COL_TILE) void edt_col_kernel(const uint8_t* __restrict__ feat, int H, int W, int* __restrict__ g2) {
    const int x = blockIdx.x * EDT_COL_TILE + threadIdx.x;
    if (x >= W) return;
    const size_t base = (size_t)blockIdx.y * H * W + x;
    int d = -1;                                         // rows since the last feature above, -1: none yet
    for (int y = 0; y < H; ++y) {
        if (feat[base + (size_t)y * W]) d = 0;
        else if (d >= 0) ++d;
        g2[base + (size_t)y * W] = d;
    }
    d = -1;
    for (int y = H - 1; y >= 0; --y) {
        const int up = g2[base + (size_t)y * W];
        if (up == 0) d = 0;
        else if (d >= 0) ++d;
        int m = up;
        if (d >= 0 && (m < 0 || d < m)) m = d;
        g2[base + (size_t)y * W] = m < 0 ? EDT_INF : m * m;
    }
}

// row pass: d2[x] = min_x' (x - x')^2 + g2[x'], integers throughout.  The scan walks outwards from x and stops once the
// horizontal part alone reaches the best value so far: every x' it skips has (x - x')^2 >= best.
__global__ __launch_bounds__(EDT_ROW_TILE) void edt_row_kernel(const int* __restrict__ g2, int H, int W, int sentinel,
                                                              int* __restrict__ d2) {
    __shared__ int row[EDT_MAX_DIM];
    const size_t base = ((size_t)blockIdx.y * H + blockIdx.x) * W;
    int any = 0;
    for (int x = threadIdx.x; x < W; x += EDT_ROW_TILE) {
        const int g = g2[base + x];
        row[x] = g;
        any |= g < EDT_INF;
    }
    if (!__syncthreads_or(any)) {       // no column has a feature, i.e. the image has none: the scan below would walk the whole row
        for (int x = threadIdx.x; x < W; x += EDT_ROW_TILE) d2[base + x] = sentinel;
        return;
    }
    for (int x = threadIdx.x; x < W; x += EDT_ROW_TILE) {
        int best = row[x];
        for (int k = 1; k < W; ++k) {
            const int kk = k * k;
            if (kk >= best) break;
            const int l = x - k, r = x + k;
            if (l < 0 && r >= W) break;
            if (l >= 0) best = min(best, kk + row[l]);
            if (r < W) best = min(best, kk + row[r]);
        }
        d2[base + x] = best >= EDT_INF ? sentinel : best;
    }
}

int edt_sentinel(int H, int W) {
    const int m = H > W ? H : W;
    return 2 * m * m;
}

// g2: (B,H,W) ints of scratch for the column distances
void edt_launch(const uint8_t* feat, int B, int H, int W, int* g2, int* d2, hipStream_t s) {
    hipLaunchKernelGGL(edt_col_kernel, dim3((W + EDT_COL_TILE - 1) / EDT_COL_TILE, B), dim3(EDT_COL_TILE), 0, s, feat, H, W, g2);
    hipLaunchKernelGGL(edt_row_kernel, dim3(H, B), dim3(EDT_ROW_TILE), 0, s, g2, H, W, edt_sentinel(H, W), d2);
}

__global__ void edt_sqrt_kernel(const int* __restrict__ d2, size_t n, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __dsqrt_rn((double)d2[i]);
}

// ---- reference edges and their distance transform ------------------------------------------------------------------------
// max over the k x k window of the in-bounds pixels (the padding of torch's max_pool2d never wins), first maximum in
// row-major order; *arg = its index y * S + x
__device__ inline float window_max(const float* __restrict__ img, int S, int y, int x, int r, int* arg) {
    const int y0 = max(y - r, 0), y1 = min(y + r, S - 1), x0 = max(x - r, 0), x1 = min(x + r, S - 1);
    float best = img[(size_t)y0 * S + x0];
    int bi = y0 * S + x0;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) {
            const float v = img[(size_t)yy * S + xx];
            if (v > best) { best = v; bi = yy * S + xx; }
        }
    *arg = bi;
    return best;
}

__global__ void ref_edges_kernel(const float* __restrict__ image_ref, int S, int ksize, float* __restrict__ edges,
                                 uint8_t* __restrict__ feat) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S * S) return;
    const size_t o = (size_t)blockIdx.y * S * S;
    int arg;
    const float e = window_max(image_ref + o, S, p / S, p % S, ksize / 2, &arg) - image_ref[o + p];
    edges[o + p] = e;
    feat[o + p] = e > 0.f;
}

__global__ void edt_power_kernel(const int* __restrict__ d2, size_t n, int quarter, double two_p, float* __restrict__ edt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = __dsqrt_rn((double)d2[i]);
    edt[i] = (float)(quarter ? __dsqrt_rn(d) : pow(d, two_p));
}

// ---- boxes, intrinsics, crops --------------------------------------------------------------------------------------------
__global__ void box_fill_kernel(int* __restrict__ box, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * 4) box[i] = (i & 3) < 2 ? INT_MAX : -1;        // x min, y min, x max, y max
}

__global__ __launch_bounds__(256) void box_kernel(const float* __restrict__ obj, int H, int W, int* __restrict__ box) {
    __shared__ int s[4];
    if (threadIdx.x < 4) s[threadIdx.x] = threadIdx.x < 2 ? INT_MAX : -1;
    __syncthreads();
    const size_t n = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && obj[(size_t)blockIdx.y * n + i] > 0.5f) {
        const int y = (int)(i / W), x = (int)(i % W);
        atomicMin(&s[0], x); atomicMin(&s[1], y); atomicMax(&s[2], x); atomicMax(&s[3], y);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s[2] >= 0) {
        int* g = box + blockIdx.y * 4 + threadIdx.x;
        if (threadIdx.x < 2) atomicMin(g, s[threadIdx.x]);
        else atomicMax(g, s[threadIdx.x]);
    }
}

// one thread per frame; double arithmetic in the order of mask2bbox, make_bbox_square, to_original_bbox and compute_K_roi
// (recon/obj_pose_roi.py), every operation rounded once (no contraction), the intrinsics rounded to float at the end
__global__ void roi_kernel(const int* __restrict__ box, const float* __restrict__ centers, int B, int H, int W, double expansion,
                           double crop_size, int net_input_size, float* __restrict__ K, double* __restrict__ box_sq,
                           int* __restrict__ valid) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int* ib = box + b * 4;
    const bool ok = ib[2] >= 0;
    double sx, sy, ss;
    if (ok) {
        const double x0 = (double)ib[0], y0 = (double)ib[1], x1 = (double)(ib[2] + 1), y1 = (double)(ib[3] + 1);
        const double w = __dsub_rn(x1, x0), hh = __dsub_rn(y1, y0);
        const double cx = __dadd_rn(x0, __ddiv_rn(w, 2.0)), cy = __dadd_rn(y0, __ddiv_rn(hh, 2.0));
        ss = __dmul_rn(fmax(w, hh), __dadd_rn(1.0, expansion));
        sx = __dsub_rn(cx, __ddiv_rn(ss, 2.0));
        sy = __dsub_rn(cy, __ddiv_rn(ss, 2.0));
    } else {                         // empty object mask: the whole image, so that the intrinsics stay finite
        sx = sy = 0.0;
        ss = (double)(H > W ? H : W);
    }
    box_sq[b * 4 + 0] = sx; box_sq[b * 4 + 1] = sy; box_sq[b * 4 + 2] = ss; box_sq[b * 4 + 3] = ss;
    valid[b] = ok;
    const double scale = __ddiv_rn(crop_size, (double)net_input_size);
    const double half = __ddiv_rn(crop_size, 2.0);
    const double ox = __dadd_rn(__dmul_rn(sx, scale), __dsub_rn((double)centers[b * 2 + 0], half));
    const double oy = __dadd_rn(__dmul_rn(sy, scale), __dsub_rn((double)centers[b * 2 + 1], half));
    const double os = __dmul_rn(ss, scale);
    const double kw = 2048.0;
    const double fx = __ddiv_rn(979.7844, kw), fy = __ddiv_rn(979.840, kw), cx = __ddiv_rn(1018.952, kw), cy = __ddiv_rn(779.486, kw);
    float* k = K + b * 9;
    k[0] = (float)__ddiv_rn(__dmul_rn(fx, kw), os); k[1] = 0.f; k[2] = (float)__ddiv_rn(__dsub_rn(__dmul_rn(cx, kw), ox), os);
    k[3] = 0.f; k[4] = (float)__ddiv_rn(__dmul_rn(fy, kw), os); k[5] = (float)__ddiv_rn(__dsub_rn(__dmul_rn(cy, kw), oy), os);
    k[6] = 0.f; k[7] = 0.f; k[8] = 1.f;
}

// bilinear tap at (px, py) in pixel coordinates, zeros outside (grid_sample, align_corners=True, padding_mode="zeros")
__device__ inline double bilinear0(const float* __restrict__ m, int H, int W, double px, double py) {
    const double fx = floor(px), fy = floor(py);
    const double wx1 = __dsub_rn(px, fx), wy1 = __dsub_rn(py, fy);
    const double wx0 = __dsub_rn(1.0, wx1), wy0 = __dsub_rn(1.0, wy1);
    // (coordinates far outside the image: every tap is out of bounds; the comparison is made in double before any conversion)
    if (!(fx >= -1.0 && fx <= (double)W && fy >= -1.0 && fy <= (double)H)) return 0.0;
    const int x0 = (int)fx, y0 = (int)fy;
    auto at = [&](int y, int x) { return (x >= 0 && x < W && y >= 0 && y < H) ? (double)m[(size_t)y * W + x] : 0.0; };
    double v = __dmul_rn(__dmul_rn(at(y0, x0), wy0), wx0);
    v = __dadd_rn(v, __dmul_rn(__dmul_rn(at(y0, x0 + 1), wy0), wx1));
    v = __dadd_rn(v, __dmul_rn(__dmul_rn(at(y0 + 1, x0), wy1), wx0));
    v = __dadd_rn(v, __dmul_rn(__dmul_rn(at(y0 + 1, x0 + 1), wy1), wx1));
    return v;
}

__global__ void crop_kernel(const float* __restrict__ person, const float* __restrict__ obj, const double* __restrict__ box_sq,
                            const int* __restrict__ valid, int H, int W, int S, float* __restrict__ image_ref,
                            float* __restrict__ keep_mask) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S * S) return;
    const int b = blockIdx.y;
    const size_t o = (size_t)b * S * S + p;
    if (!valid[b]) {
        image_ref[o] = 0.f;
        keep_mask[o] = 0.f;
        return;
    }
    const double x0 = box_sq[b * 4], y0 = box_sq[b * 4 + 1];
    const double x1 = __dadd_rn(x0, box_sq[b * 4 + 2]), y1 = __dadd_rn(y0, box_sq[b * 4 + 3]);
    // crop_and_resize: x0 + (i + 0.5) * (x1 - x0) / size - 0.5
    const double px = __dsub_rn(__dadd_rn(x0, __ddiv_rn(__dmul_rn(__dadd_rn((double)(p % S), 0.5), __dsub_rn(x1, x0)), (double)S)), 0.5);
    const double py = __dsub_rn(__dadd_rn(y0, __ddiv_rn(__dmul_rn(__dadd_rn((double)(p / S), 0.5), __dsub_rn(y1, y0)), (double)S)), 0.5);
    const size_t f = (size_t)b * H * W;
    const bool fore = bilinear0(obj + f, H, W, px, py) >= 0.5;
    const bool ps = bilinear0(person + f, H, W, px, py) >= 0.5;
    image_ref[o] = fore ? 1.f : 0.f;
    keep_mask[o] = (fore || !ps) ? 1.f : 0.f;       // cvt_masks: the rendering counts on the object and on free background
}

// ---- edge term -----------------------------------------------------------------------------------------------------------
// forward: one pixel per thread, a tree over the block's EDGE_TILE terms (8 levels), one partial per block
__global__ __launch_bounds__(EDGE_TILE) void edge_fwd_kernel(const float* __restrict__ image, const float* __restrict__ weight,
                                                            int S, int ksize, int* __restrict__ argmax,
                                                            float* __restrict__ partial) {
    __shared__ float s[EDGE_TILE];
    const int p = blockIdx.x * EDGE_TILE + threadIdx.x;
    const size_t o = (size_t)blockIdx.y * S * S;
    float term = 0.f;
    if (p < S * S) {
        int arg;
        const float m = window_max(image + o, S, p / S, p % S, ksize / 2, &arg);
        argmax[o + p] = arg;
        term = __fmul_rn(__fsub_rn(m, image[o + p]), weight[o + p]);
    }
    s[threadIdx.x] = term;
    __syncthreads();
    for (int k = EDGE_TILE / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s[0];
}

// the frame's partials: thread t adds partials t, t + EDGE_TILE, ... in order, then the same tree
__global__ __launch_bounds__(EDGE_TILE) void edge_sum_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ out) {
    __shared__ float s[EDGE_TILE];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nblk; i += EDGE_TILE) acc += partial[(size_t)blockIdx.x * nblk + i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int k = EDGE_TILE / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// backward, gather form: the pixels q whose window holds p are those of p's own window; row-major order
__global__ void edge_bwd_kernel(const float* __restrict__ weight, const int* __restrict__ argmax, const float* __restrict__ g,
                                int S, int ksize, float* __restrict__ g_image) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S * S) return;
    const size_t o = (size_t)blockIdx.y * S * S;
    const int r = ksize / 2, y = p / S, x = p % S;
    const int y0 = max(y - r, 0), y1 = min(y + r, S - 1), x0 = max(x - r, 0), x1 = min(x + r, S - 1);
    float acc = 0.f;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx)
            if (argmax[o + (size_t)yy * S + xx] == p) acc += weight[o + (size_t)yy * S + xx];
    g_image[o + p] = __fmul_rn(g[blockIdx.y], __fsub_rn(acc, weight[o + p]));
}

bool edt_sizes_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && H <= EDT_MAX_DIM && W <= EDT_MAX_DIM && B <= 65535; }

// workspace of chore_sil_edge_edt: feature bytes | column distances | squared distances
struct EdgeEdtWs { uint8_t* feat; int* g2; int* d2; size_t bytes; };
EdgeEdtWs edge_edt_ws(void* base, int B, int S) {
    const size_t n = (size_t)B * S * S;
    WsCarver c(base);
    return {c.take<uint8_t>(n), c.take<int>(n), c.take<int>(n), c.bytes};
}

bool edge_sizes_ok(int B, int S, int ksize) {
    return B > 0 && S > 0 && S <= EDT_MAX_DIM && B <= 65535 && ksize >= 1 && (ksize & 1) && ksize <= EDGE_MAX_K;
}

}  // namespace

extern "C" size_t chore_edt_workspace_bytes(int B, int H, int W) {
    return edt_sizes_ok(B, H, W) ? ws_align(sizeof(int) * (size_t)B * H * W) : 0;
}

extern "C" int chore_edt_sq(chore_handle* h, const uint8_t* feature, int B, int H, int W, int* d2, void* workspace,
                            chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!feature || !d2 || !workspace) CHORE_FAIL(h, CHORE_EINVAL, "chore_edt_sq: null argument");
    if (!edt_sizes_ok(B, H, W))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_edt_sq: bad sizes B=%d H=%d W=%d (H, W <= %d)", B, H, W, EDT_MAX_DIM);
    hipStream_t s = (hipStream_t)stream;
    edt_launch(feature, B, H, W, (int*)workspace, d2, s);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" int chore_edt_sqrt_f64(chore_handle* h, const int* d2, size_t n, double* out, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!d2 || !out) CHORE_FAIL(h, CHORE_EINVAL, "chore_edt_sqrt_f64: null argument");
    if (n == 0 || n > ((size_t)1 << 38)) CHORE_FAIL(h, CHORE_EINVAL, "chore_edt_sqrt_f64: bad size %zu", n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(edt_sqrt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d2, n, out);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" int chore_edt_tiles(int* col_tile, int* row_tile, int* max_dim) {
    if (col_tile) *col_tile = EDT_COL_TILE;
    if (row_tile) *row_tile = EDT_ROW_TILE;
    if (max_dim) *max_dim = EDT_MAX_DIM;
    return CHORE_OK;
}

extern "C" size_t chore_sil_edge_edt_workspace_bytes(int B, int S) {
    return edt_sizes_ok(B, S, S) ? edge_edt_ws(nullptr, B, S).bytes : 0;
}

extern "C" int chore_sil_edge_edt(chore_handle* h, const float* image_ref, int B, int S, int ksize, float power, float* edges,
                                  float* edt, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!image_ref || !edges || !edt || !workspace) CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_edge_edt: null argument");
    if (!edge_sizes_ok(B, S, ksize) || !(power > 0.f))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_edge_edt: bad sizes B=%d S=%d ksize=%d power=%g", B, S, ksize, (double)power);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * S * S;
    const EdgeEdtWs w = edge_edt_ws(workspace, B, S);
    hipLaunchKernelGGL(ref_edges_kernel, dim3((S * S + 255) / 256, B), dim3(256), 0, s, image_ref, S, ksize, edges, w.feat);
    edt_launch(w.feat, B, S, S, w.g2, w.d2, s);
    hipLaunchKernelGGL(edt_power_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.d2, n, power == 0.25f ? 1 : 0,
                       2.0 * (double)power, edt);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" size_t chore_sil_targets_workspace_bytes(int B) {
    return B > 0 ? ws_align(sizeof(int) * 4 * (size_t)B) : 0;
}

extern "C" int chore_sil_targets(chore_handle* h, const float* person, const float* obj, const float* crop_centers, int B, int H,
                                 int W, int S, double expansion, double crop_size, int net_input_size, float* image_ref,
                                 float* keep_mask, float* K, double* box_sq, int* valid, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!person || !obj || !crop_centers || !image_ref || !keep_mask || !K || !box_sq || !valid || !workspace)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_targets: null argument");
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > 32768 || W > 32768 || S <= 0 || S > EDT_MAX_DIM || net_input_size <= 0 ||
        !(crop_size > 0.0) || !(expansion > -1.0))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_targets: bad sizes B=%d H=%d W=%d S=%d", B, H, W, S);
    hipStream_t s = (hipStream_t)stream;
    int* box = (int*)workspace;
    hipLaunchKernelGGL(box_fill_kernel, dim3((B * 4 + 255) / 256), dim3(256), 0, s, box, B);
    hipLaunchKernelGGL(box_kernel, dim3((unsigned)(((size_t)H * W + 255) / 256), B), dim3(256), 0, s, obj, H, W, box);
    hipLaunchKernelGGL(roi_kernel, dim3((B + 63) / 64), dim3(64), 0, s, box, crop_centers, B, H, W, expansion, crop_size,
                       net_input_size, K, box_sq, valid);
    hipLaunchKernelGGL(crop_kernel, dim3((S * S + 255) / 256, B), dim3(256), 0, s, person, obj, box_sq, valid, H, W, S, image_ref,
                       keep_mask);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

// one float per block of the forward
extern "C" size_t chore_sil_edge_workspace_bytes(int B, int S) {
    if (B <= 0 || S <= 0 || S > EDT_MAX_DIM || B > 65535) return 0;
    return ws_align(sizeof(float) * (size_t)B * ((S * S + EDGE_TILE - 1) / EDGE_TILE));
}

extern "C" int chore_sil_edge_fwd(chore_handle* h, const float* image, const float* weight, int B, int S, int ksize,
                                  float* per_frame_sum, int* argmax, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!image || !weight || !per_frame_sum || !argmax || !workspace) CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_edge_fwd: null argument");
    if (!edge_sizes_ok(B, S, ksize)) CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_edge_fwd: bad sizes B=%d S=%d ksize=%d", B, S, ksize);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (S * S + EDGE_TILE - 1) / EDGE_TILE;
    hipLaunchKernelGGL(edge_fwd_kernel, dim3(nblk, B), dim3(EDGE_TILE), 0, s, image, weight, S, ksize, argmax, (float*)workspace);
    hipLaunchKernelGGL(edge_sum_kernel, dim3(B), dim3(EDGE_TILE), 0, s, (const float*)workspace, nblk, per_frame_sum);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" int chore_sil_edge_bwd(chore_handle* h, const float* weight, const int* argmax, const float* g_per_frame, int B, int S,
                                  int ksize, float* g_image, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!weight || !argmax || !g_per_frame || !g_image) CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_edge_bwd: null argument");
    if (!edge_sizes_ok(B, S, ksize)) CHORE_FAIL(h, CHORE_EINVAL, "chore_sil_edge_bwd: bad sizes B=%d S=%d ksize=%d", B, S, ksize);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(edge_bwd_kernel, dim3((S * S + 255) / 256, B), dim3(256), 0, s, weight, argmax, g_per_frame, S, ksize, g_image);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
