// raster_common.h -- what the silhouette rasteriser (silhouette.hip) and the colour / depth rasteriser (render.hip,
// render_bwd.hip, and through render_common.h scene.hip and instances.hip) share: the per-triangle setup and the per-sample
// hit rule of neural_renderer's forward_face_index_map (external/neural_renderer/neural_renderer/cuda/rasterize_cuda_kernel.cu:
// 24-215), and the edge walk of its backward_pixel_map (:290-549).  All kernels evaluate these very expressions (explicit
// __fmul_rn, fixed association, -ffp-contract=off), so the face that wins a sample is the same bit for bit in them, and so is the
// alpha term of the pixel-map gradient.  Also here, once for the family: the setup kernel with its launch (raster_setup_kernel,
// raster_setup; binning or not) and the in-order compaction of a workgroup's flags (raster_compact).
#pragma once
#include "common.h"

namespace {

struct TriSetup {            // per (image, triangle)
    float f[9];              // projected vertices: x0 y0 z0 x1 y1 z1 x2 y2 z2 (normalised [-1,1] + depth)
    float inv[9];            // pixel-space inverse (barycentric weights = inv * (xi, yi, 1))
    int x0, x1, y0, y1;      // inclusive pixel bounding box, x0 > x1 if the triangle is culled
};

__device__ __forceinline__ bool tri_backside(const float* f) {
    return __fmul_rn(f[7] - f[1], f[3] - f[0]) < __fmul_rn(f[4] - f[1], f[6] - f[0]);
}

// t.f is filled by the caller; cull, inverse and box for an image of size x size pixels
__device__ __forceinline__ void tri_setup(TriSetup& t, int size) {
    t.x0 = 1; t.x1 = 0; t.y0 = 1; t.y1 = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) t.inv[k] = 0.f;
    if (!tri_backside(t.f)) {
        const float S = (float)size;
        float p[3][2];
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
            for (int d = 0; d < 2; ++d) p[v][d] = 0.5f * ((t.f[3 * v + d] * S + S) - 1.0f);
        const float den = (p[2][0] * (p[0][1] - p[1][1]) + p[0][0] * (p[1][1] - p[2][1])) + p[1][0] * (p[2][1] - p[0][1]);
        const float m[9] = {p[1][1] - p[2][1], p[2][0] - p[1][0], p[1][0] * p[2][1] - p[2][0] * p[1][1],
                            p[2][1] - p[0][1], p[0][0] - p[2][0], p[2][0] * p[0][1] - p[0][0] * p[2][1],
                            p[0][1] - p[1][1], p[1][0] - p[0][0], p[0][0] * p[1][1] - p[1][0] * p[0][1]};
#pragma unroll
        for (int k = 0; k < 9; ++k) t.inv[k] = m[k] / den;
        // conservative box: pixel centres inside the triangle lie within [min, max] of the vertex pixel coordinates;
        // one pixel of slack covers the rounding of the normalised-coordinate inside test
        const float xmin = fminf(fminf(p[0][0], p[1][0]), p[2][0]), xmax = fmaxf(fmaxf(p[0][0], p[1][0]), p[2][0]);
        const float ymin = fminf(fminf(p[0][1], p[1][1]), p[2][1]), ymax = fmaxf(fmaxf(p[0][1], p[1][1]), p[2][1]);
        if (xmin == xmin && ymin == ymin && xmax == xmax && ymax == ymax) {   // not NaN
            t.x0 = (int)fmaxf(floorf(xmin) - 1.f, 0.f);
            t.y0 = (int)fmaxf(floorf(ymin) - 1.f, 0.f);
            t.x1 = (int)fminf(ceilf(xmax) + 1.f, S - 1.f);
            t.y1 = (int)fminf(ceilf(ymax) + 1.f, S - 1.f);
        }
    }
}

constexpr int RB_BIN = 256;          // coarse bin edge in samples: at most 16 x 16 bins (size * ssaa <= 4096)
__host__ __device__ inline int rb_bins(int S) { return (S + RB_BIN - 1) / RB_BIN; }

// The one setup kernel of the family: thread = (image, triangle) -> its TriSetup for an S x S grid.  BIN: also append every
// front-facing, in-view triangle to the lists of the coarse bins its box meets (count [B*nb*nb], zeroed by the caller; list
// [B*nb*nb][F]).  Without BIN the two pointers are not read.
template <bool BIN>
__global__ __launch_bounds__(256) void raster_setup_kernel(const float* __restrict__ faces, int B, int F, int S,
                                                           TriSetup* __restrict__ ts, int* __restrict__ count,
                                                           int* __restrict__ list) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * F) return;
    TriSetup t;
#pragma unroll
    for (int k = 0; k < 9; ++k) t.f[k] = faces[(size_t)i * 9 + k];
    tri_setup(t, S);
    ts[i] = t;
    if constexpr (BIN) {
        // culled triangles have x0 > x1; a triangle outside the view ends up with an empty clamped box as well
        if (t.x0 > t.x1 || t.y0 > t.y1) return;
        const int b = i / F, fn = i - b * F;
        const int nb = rb_bins(S);
        // 0 <= x0 <= x1 <= S - 1 here, so every bin index is inside [0, nb)
        for (int by = t.y0 / RB_BIN; by <= t.y1 / RB_BIN; ++by)
            for (int bx = t.x0 / RB_BIN; bx <= t.x1 / RB_BIN; ++bx) {
                const size_t bin = ((size_t)b * nb + by) * nb + bx;
                const int slot = atomicAdd(&count[bin], 1);     // < F: a triangle enters a bin's list at most once
                list[bin * F + slot] = fn;
            }
    }
}
// its launch on stream s; count == NULL: no binning (the silhouette and the render backward)
inline void raster_setup(hipStream_t s, const float* tri, int B, int F, int S, TriSetup* ts, int* count = nullptr,
                         int* list = nullptr) {
    const dim3 grid((B * F + 255) / 256);
    if (count) hipLaunchKernelGGL(raster_setup_kernel<true>, grid, dim3(256), 0, s, tri, B, F, S, ts, count, list);
    else hipLaunchKernelGGL(raster_setup_kernel<false>, grid, dim3(256), 0, s, tri, B, F, S, ts, count, list);
}

// Compaction in thread order over a 256-thread workgroup (keeps the z-buffer order deterministic): ballots and a prefix over the
// four waves (one thread walking the 256 flags was 2.4 us per chunk, most of the silhouette kernel).  Every thread calls it; the
// values of the threads with `keep` go to out[0, n) and n is returned.  wcnt: int[4] of LDS; wv, ln: the caller's wave and lane
// (threadIdx.x >> 6, & 63: the walk has them in registers already, and computing them here again costs its tile kernels two VGPRs).
// Both barriers are inside: out and n are valid for every thread afterwards, and wcnt may be written again.
__device__ __forceinline__ int raster_compact(bool keep, int value, int* out, int* wcnt, int wv, int ln) {
    const unsigned long long mb = __ballot(keep);
    if (ln == 0) wcnt[wv] = __popcll(mb);
    __syncthreads();
    {
        int base = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) base += q < wv ? wcnt[q] : 0;
        if (keep) out[base + __popcll(mb & ((1ull << ln) - 1ull))] = value;
    }
    const int nh = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
    __syncthreads();
    return nh;
}

// normalised coordinate of the centre of pixel i of `size` (evaluated in double, stored as float, like the reference)
__device__ __forceinline__ float raster_centre(int i, int size) { return (float)((2.0 * i + 1 - size) / size); }

// the clamped and renormalised barycentric weights of the pixel (xf, yf) under the pixel-space inverse m, and the
// perspective-correct depth zp they give on the triangle f: what a hit keeps, and what the backward rebuilds for a winner
__device__ __forceinline__ void raster_weights(const float* f, const float* m, float xf, float yf, float* w, float& zp) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = (m[3 * k] * xf + m[3 * k + 1] * yf) + m[3 * k + 2];
        v = fminf(fmaxf(v, 0.f), 1.f);     // NaN -> 0 like CUDA's fmax/fmin
        w[k] = v;
    }
    const float ws = (w[0] + w[1]) + w[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = w[k] / ws;
    zp = 1.0f / ((w[0] / f[2] + w[1] / f[5]) + w[2] / f[8]);
}

// does the sample (xp, yp) normalised / (xf, yf) pixel hit the front-facing triangle (f, inverse m)?  On a hit: the clamped
// and renormalised barycentric weights and the perspective-correct depth zp, already checked against near / far.
__device__ __forceinline__ bool raster_hit(const float* f, const float* m, float xp, float yp, float xf, float yf, float near,
                                           float far, float* w, float& zp) {
    if (__fmul_rn(yp - f[1], f[3] - f[0]) < __fmul_rn(xp - f[0], f[4] - f[1]) ||
        __fmul_rn(yp - f[4], f[6] - f[3]) < __fmul_rn(xp - f[3], f[7] - f[4]) ||
        __fmul_rn(yp - f[7], f[0] - f[6]) < __fmul_rn(xp - f[6], f[1] - f[7]))
        return false;
    raster_weights(f, m, xf, yf, w, zp);
    return !(zp <= near || far <= zp);
}

// ---- the backward of the depth map (rasterize_cuda_kernel.cu:588-638), shared by render_bwd.hip's gather and ordinal_depth.hip.
// A sample the face won, with its weights w and depth zp, and the upstream gradient g of that depth: A_k += g zp^2 w_k
__device__ __forceinline__ void raster_depth_bwd_sample(float g, const float* w, float zp, float* A) {
    const float a = g * (zp * zp);
#pragma unroll
    for (int k = 0; k < 3; ++k) A[k] += a * w[k];
}
// the face's nine components from its three sums: d z_k = A_k / z_k^2, d (x, y)_k = -tmp_l A_k S / 2, tmp_l = sum_m -inv[3 m + l] / z_m
__device__ __forceinline__ void raster_depth_bwd_face(const TriSetup& t, const float* A, int S, float* g9) {
    float tmp[2] = {0.f, 0.f};
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
        for (int k = 0; k < 3; ++k) tmp[l] += -t.inv[3 * k + l] / t.f[3 * k + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // a == 0: no sample of this triangle carries a depth gradient (a zero-area triangle has no finite inverse)
        const float a = A[k], z = t.f[3 * k + 2];
        g9[3 * k + 2] = a == 0.f ? 0.f : a / (z * z);
#pragma unroll
        for (int l = 0; l < 2; ++l) g9[3 * k + l] = a == 0.f ? 0.f : -a * tmp[l] * (float)S / 2.f;
    }
}
// The pixels a face won, walked by its 256-thread workgroup: the aligned 16 x 16 tiles that the face's box meets (exactly where the
// forward tested it), tiles in row-major order, thread = one pixel of a tile.  fn(q, x, y, w, zp) for every pixel (x, y) of the
// S x S winner map `fim` (ONE image) whose winner is `face`: q = y * S + x, w and zp its weights and depth rebuilt with the
// forward's expressions.  Returns whether this THREAD met one.  The box must not be empty (x0 <= x1, y0 <= y1).
template <class Fn>
__device__ __forceinline__ int raster_for_each_won_pixel(const TriSetup& t, const int* __restrict__ fim, int face, int S, Fn&& fn) {
    const int bx0 = t.x0 & ~15, bx1 = min(t.x1 | 15, S - 1), by0 = t.y0 & ~15, by1 = min(t.y1 | 15, S - 1);
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    int mine = 0;
    for (int ty = by0; ty <= by1; ty += 16)
        for (int tx = bx0; tx <= bx1; tx += 16) {
            const int x = tx + lx, y = ty + ly;
            if (x > bx1 || y > by1) continue;
            const size_t q = (size_t)y * S + x;
            if (fim[q] != face) continue;
            mine = 1;
            float w[3], zp;
            raster_weights(t.f, t.inv, (float)x, (float)y, w, zp);
            fn(q, x, y, w, zp);
        }
    return mine;
}
// The sums of a 256-thread workgroup over N per-thread values: a fixed butterfly per wave, then the four waves in order.  Every
// thread calls it; red[0][k] holds sum k afterwards, for every thread (both barriers are inside).
template <int N>
__device__ __forceinline__ void raster_wg_sum(const float* acc, float (*red)[N]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) red[0][threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    __syncthreads();
}

// ---- the backward of the pixel map (rasterize_cuda_kernel.cu:290-549): the edge walk, shared by silhouette.hip (alpha
// alone) and render_bwd.hip (alpha + rgb).  An image type Im says what a pixel holds and what it contributes:
//   int size;  size_t at(axis, d0, d1): the pixel with coordinate d0 along the walk axis and d1 across it;
//   int face(q): its winning face;  Ref ref(q): its values as the 'in' / 'out' pixel of a crossing;
//   Px load(q): its values and upstream gradients;  float diff(px, ref): diff_grad, summed over the channels BEFORE the gate.
constexpr int EDGE_U = 8;     // pixels of a line whose loads are in flight together
// One walk along edge (P0 -> P1) of triangle fn on one axis; P2 is the opposite vertex.  u = coordinate along the walk
// axis, v = across it.  Adds to g0 / g1 (the gradient of P0 / P1 along v).  The 64 lanes of a wave share one walk: lane l
// takes the positions d0_from + l, + 64, ... along the edge.
template <class Im>
__device__ void raster_edge_walk(const Im& im, int fn, int axis, float u0, float v0, float u1, float v1, float u2, float v2,
                                 float eps, int lane, float& g0, float& g1) {
    const int size = im.size;
    const float S = (float)size;
    int direction;
    if (axis == 0) direction = (u0 < u1) ? -1 : 1;
    else direction = (u0 < u1) ? 1 : -1;
    const int d0_from = (int)fmaxf(ceilf(fminf(u0, u1)), 0.f);
    const int d0_to = (int)fminf(fmaxf(u0, u1), S - 1.f);
    for (int d0 = d0_from + lane; d0 <= d0_to; d0 += 64) {
        const float fd0 = (float)d0;
        const float cross = (v1 - v0) / (u1 - u0) * (fd0 - u0) + v0;
        if (!(fabsf(cross) <= 3.0e38f)) continue;          // non-finite: degenerate edge
        const int d1_in = direction > 0 ? (int)floorf(cross) : (int)ceilf(cross);
        const int d1_out = d1_in + direction;
        if (d1_in < 0 || d1_in >= size || d1_out < 0 || d1_out >= size) continue;
        const typename Im::Ref r_in = im.ref(im.at(axis, d0, d1_in)), r_out = im.ref(im.at(axis, d0, d1_out));
        auto push = [&](int d1, float diff) {
            if (!(diff > 0.f)) return;
            const float t = ((float)d1 - cross);
            if (u1 != fd0) {
                float dist = (u1 - u0) / (u1 - fd0) * t * 2.0f / S;
                dist = dist > 0.f ? dist + eps : dist - eps;
                g0 -= diff / dist;
            }
            if (u0 != fd0) {
                float dist = (u1 - u0) / (fd0 - u0) * t * 2.0f / S;
                dist = dist > 0.f ? dist + eps : dist - eps;
                g1 -= diff / dist;
            }
        };
        if (im.face(im.at(axis, d0, d1_in)) == fn) {         // 'out': beyond the edge up to the image border
            const int lim = direction > 0 ? size - 1 : 0;
            const int lo = max(min(d1_out, lim), 0), hi = min(max(d1_out, lim), size - 1);
            for (int d1 = lo; d1 <= hi; d1 += EDGE_U) {     // EDGE_U pixels' loads requested together, pushed in pixel order
                typename Im::Px px[EDGE_U];
#pragma unroll
                for (int u = 0; u < EDGE_U; ++u) px[u] = im.load(im.at(axis, d0, min(d1 + u, hi)));
#pragma unroll
                for (int u = 0; u < EDGE_U; ++u)
                    if (d1 + u <= hi) push(d1 + u, im.diff(px[u], r_in));
            }
        }
        float c2;                                            // 'in': this face's pixels up to the opposite edge
        if ((fd0 - u0) * (fd0 - u2) < 0.f) c2 = (v2 - v0) / (u2 - u0) * (fd0 - u0) + v0;
        else c2 = (v1 - v2) / (u1 - u2) * (fd0 - u2) + v2;
        if (!(fabsf(c2) <= 3.0e38f)) continue;
        const int lim = direction > 0 ? (int)ceilf(c2) : (int)floorf(c2);
        const int lo = max(min(d1_in, lim), 0), hi = min(max(d1_in, lim), size - 1);
        for (int d1 = lo; d1 <= hi; d1 += EDGE_U) {
            typename Im::Px px[EDGE_U];
            int fm[EDGE_U];
#pragma unroll
            for (int u = 0; u < EDGE_U; ++u) {
                const size_t q = im.at(axis, d0, min(d1 + u, hi));
                fm[u] = im.face(q); px[u] = im.load(q);
            }
#pragma unroll
            for (int u = 0; u < EDGE_U; ++u)
                if (d1 + u <= hi && fm[u] == fn) push(d1 + u, im.diff(px[u], r_out));
        }
    }
}

// The six walks of one front-facing triangle f (index fn of image im) by a workgroup of 384 threads: a wave takes one
// (edge, axis) walk, a lane one position along the edge.  The reference gives a whole triangle to ONE thread, whose six walks
// of up to `size` positions x up to `size` pixels each are a serial chain of tens of thousands of dependent loads.  The
// per-lane partial sums are combined with a fixed butterfly and the six walks in the reference's order (edges 0, 1, 2, axis 0
// before axis 1), so the result is deterministic; it differs from the serial sum by fp32 round-off only.  Every thread of
// the workgroup must call it; thread 0 stores the nine components (depth components zero) to g9.  part: LDS.
template <class Im>
__device__ __forceinline__ void raster_pixel_map_bwd(const Im& im, const float* f, int fn, bool back, float eps,
                                                     float (&part)[6][2], float* __restrict__ g9) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float g0 = 0.f, g1 = 0.f;
    if (!back) {
        const float S = (float)im.size;
        float px[3], py[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            px[v] = 0.5f * ((f[3 * v] * S + S) - 1.0f);
            py[v] = 0.5f * ((f[3 * v + 1] * S + S) - 1.0f);
        }
        const int e = wave >> 1, axis = wave & 1;
        const int i0 = e, i1 = (e + 1) % 3, i2 = (e + 2) % 3;
        // axis 0: walk x, the gradient goes to y; axis 1: walk y, the gradient goes to x
        if (axis == 0) raster_edge_walk(im, fn, 0, px[i0], py[i0], px[i1], py[i1], px[i2], py[i2], eps, lane, g0, g1);
        else raster_edge_walk(im, fn, 1, py[i0], px[i0], py[i1], px[i1], py[i2], px[i2], eps, lane, g0, g1);
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            g0 += __shfl_xor(g0, o);
            g1 += __shfl_xor(g1, o);
        }
    }
    if (lane == 0) { part[wave][0] = g0; part[wave][1] = g1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float g[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) g[k] = 0.f;
        for (int e = 0; e < 3; ++e) {
            const int i0 = e, i1 = (e + 1) % 3;
            g[3 * i0 + 1] += part[2 * e][0];
            g[3 * i1 + 1] += part[2 * e][1];
            g[3 * i0 + 0] += part[2 * e + 1][0];
            g[3 * i1 + 0] += part[2 * e + 1][1];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) g9[k] = g[k];
    }
}

}  // namespace
