// splat.hip -- point clouds as shaded discs: colour / depth / coverage, forward only, for the fit's debug views.
//
// The point primitive next to render.hip's triangles.  A point [u, v, depth] with a radius in output pixels covers the
// samples of the size * ssaa grid whose centre lies inside its disc; the nearest point wins a sample (smallest depth, then
// smallest index), the sample is shaded like a small sphere, and the image is resolved exactly as chore_render_fwd resolves
// its own (row flip, mean over the ssaa x ssaa samples of rgb, depth and alpha alike).
//   * one 64-bit key per sample: the depth's bits (mapped so that unsigned order = float order) above the point index.
//     splat_kernel takes a sample with an integer atomicMin, which is exact and commutative, so the keys after the pass
//     depend on the SET of points only: a permuted cloud, a second call and a graph replay give the same bits.  No float
//     atomics anywhere.
//   * work distribution: a lane loads one point.  Discs of at most SP_LANE_RS samples radius (a box of <= 8 x 8 with its slack)
//     are drawn by that lane; every larger disc is then drawn by the whole wave, 64 samples of its box per step, one disc
//     after the other (the wave's ballot of "large" lanes is wave-uniform).  A 64-sample marker (132 x 132 box at most) therefore
//     costs its wave 273 steps of 64 lanes, never one lane 17 424 steps beside 3-sample neighbours.
//   * resolve_kernel: a lane owns one output pixel = ssaa x ssaa keys (one 16-byte load per sample row), recomputes d2 of
//     each winner with the very expressions of the coverage test, shades, averages, flips the row, stores channel-first.
// Every expression that decides coverage is spelled with __fmul_rn / __fadd_rn / __fsub_rn in a fixed association (and the
// library is built with -ffp-contract=off), so tests/splat_ref.py reproduces the winners in numpy float32.
#include "common.h"

namespace {

constexpr float SP_MAX_RS = 64.f;    // radii are clamped to this many samples
constexpr float SP_LANE_RS = 2.f;    // up to here a disc is drawn by the lane that loaded it
constexpr unsigned long long SP_EMPTY = ~0ull;

// sample-space position of a normalised coordinate: raster_common.h's vertex expression, 0.5f * ((u * S + S) - 1.0f)
__device__ __forceinline__ float sp_pos(float u, float Sf) {
    return __fmul_rn(0.5f, __fsub_rn(__fadd_rn(__fmul_rn(u, Sf), Sf), 1.0f));
}

struct SplatPoint {
    float px, py, z, rs;
};

// point i of the flattened (B*N) list; false = skipped (NaN, radius <= 0, outside the depth range)
__device__ __forceinline__ bool sp_load(const float* __restrict__ pts, const float* __restrict__ radius, float radius_px,
                                        int SS, float Sf, float near, float far, size_t i, SplatPoint& p) {
    const float u = pts[3 * i], v = pts[3 * i + 1], z = pts[3 * i + 2];
    const float r = radius ? radius[i] : radius_px;
    if (u != u || v != v || z != z || r != r) return false;
    if (r <= 0.f || z <= near || far <= z) return false;
    p.rs = fminf(__fmul_rn(r, (float)SS), SP_MAX_RS);
    p.px = sp_pos(u, Sf);
    p.py = sp_pos(v, Sf);
    p.z = z;
    return true;
}

__device__ __forceinline__ float sp_d2(int i, int j, float px, float py) {
    const float dx = __fsub_rn((float)i, px), dy = __fsub_rn((float)j, py);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

// depth bits above the index; the map makes unsigned order equal float order for every non-NaN depth (-0 is stored as +0,
// which compares equal to it), so min over keys = smallest depth, then smallest index
__device__ __forceinline__ unsigned long long sp_key(float z, unsigned n) {
    unsigned b = __float_as_uint(z == 0.f ? 0.f : z);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 32) | n;
}

// the inclusive sample box that can hold covered samples, one sample of slack on every side for the rounding of px -+ rs
// (the coverage test decides); false = nothing inside the image.  Clamped in float, so a far-away point never overflows int.
__device__ __forceinline__ bool sp_box(const SplatPoint& p, int S, int& x0, int& x1, int& y0, int& y1) {
    const float hi = (float)(S - 1);
    const float fx0 = fmaxf(__fsub_rn(floorf(__fsub_rn(p.px, p.rs)), 1.f), 0.f), fx1 = fminf(__fadd_rn(ceilf(__fadd_rn(p.px, p.rs)), 1.f), hi);
    const float fy0 = fmaxf(__fsub_rn(floorf(__fsub_rn(p.py, p.rs)), 1.f), 0.f), fy1 = fminf(__fadd_rn(ceilf(__fadd_rn(p.py, p.rs)), 1.f), hi);
    if (!(fx0 <= fx1 && fy0 <= fy1)) return false;
    x0 = (int)fx0; x1 = (int)fx1; y0 = (int)fy0; y1 = (int)fy1;
    return true;
}

// every key = SP_EMPTY.  A kernel, not hipMemsetAsync: the call is recorded into hipGraphs, where byte-memset nodes replay
// unreliably (GPU memory faults; contact.hip fills its workspace with a kernel for the same reason).  16-byte stores; n keys.
__global__ __launch_bounds__(256) void splat_clear_kernel(unsigned long long* __restrict__ keys, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (2 * i + 1 < n)
        reinterpret_cast<ulonglong2*>(keys)[i] = make_ulonglong2(SP_EMPTY, SP_EMPTY);
    else if (2 * i < n)
        keys[2 * i] = SP_EMPTY;
}

// One wave per workgroup: the wave is the unit of work here (nothing is shared between waves), so a debug cloud of ~17 000 points
// is 264 workgroups, one per CU.  Measured against 256 threads per workgroup at that size: no difference (75.7 vs 71.7 us on two
// machines, profiles/splat_bench.txt) -- the kernel is as long as its longest wave, the one that draws a marker.
constexpr int SP_BLOCK = 64;
__global__ __launch_bounds__(SP_BLOCK) void splat_kernel(const float* __restrict__ pts, const float* __restrict__ radius,
                                                    float radius_px, int total, int N, int S, int SS, float near, float far,
                                                    unsigned long long* __restrict__ keys) {
    const int g = blockIdx.x * SP_BLOCK + threadIdx.x;
    const int ln = threadIdx.x;
    const float Sf = (float)S;
    SplatPoint p = {0.f, 0.f, 0.f, 0.f};
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    bool ok = g < total && sp_load(pts, radius, radius_px, SS, Sf, near, far, (size_t)g, p);
    ok = ok && sp_box(p, S, x0, x1, y0, y1);
    const int b = ok ? g / N : 0;
    const unsigned n = (unsigned)(g - b * N);
    const bool big = ok && p.rs > SP_LANE_RS;
    if (ok && !big) {
        const float rs2 = __fmul_rn(p.rs, p.rs);
        const unsigned long long key = sp_key(p.z, n);
        unsigned long long* kb = keys + (size_t)b * S * S;
        for (int j = y0; j <= y1; ++j)
            for (int i = x0; i <= x1; ++i)
                if (sp_d2(i, j, p.px, p.py) <= rs2) atomicMin(&kb[(size_t)j * S + i], key);
    }
    // the large discs of this wave, one after the other, 64 samples of the box per step
    unsigned long long m = __ballot(big);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float qx = __shfl(p.px, src), qy = __shfl(p.py, src), qz = __shfl(p.z, src), qr = __shfl(p.rs, src);
        const int bx0 = __shfl(x0, src), bx1 = __shfl(x1, src), by0 = __shfl(y0, src), by1 = __shfl(y1, src);
        const int qb = __shfl(b, src);
        const unsigned qn = (unsigned)__shfl((int)n, src);
        const float rs2 = __fmul_rn(qr, qr);
        const unsigned long long key = sp_key(qz, qn);
        unsigned long long* kb = keys + (size_t)qb * S * S;
        const int w = bx1 - bx0 + 1, cnt = w * (by1 - by0 + 1);      // <= 132 * 132
        for (int e = ln; e < cnt; e += 64) {
            const int r = e / w, c = e - r * w;
            const int i = bx0 + c, j = by0 + r;                       // inside [0, S) by sp_box
            if (sp_d2(i, j, qx, qy) <= rs2) atomicMin(&kb[(size_t)j * S + i], key);
        }
    }
}

template <int SS>
__global__ __launch_bounds__(256) void splat_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                            const float* __restrict__ pts, const float* __restrict__ colors,
                                                            const float* __restrict__ radius, float radius_px, int N, int size,
                                                            float ambient, float near, float far, float bg0, float bg1,
                                                            float bg2, float* __restrict__ rgb, float* __restrict__ depth_out,
                                                            float* __restrict__ alpha_out, int* __restrict__ sample_point_index) {
    constexpr int NS = SS * SS;
    const int S = size * SS;
    const int b = blockIdx.z;
    const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);   // rows not flipped
    if (px >= size || py >= size) return;
    const float Sf = (float)S;
    const float direct = __fsub_rn(1.f, ambient);
    const unsigned long long* kb = keys + (size_t)b * S * S;

    unsigned long long k[NS];
#pragma unroll
    for (int sy = 0; sy < SS; ++sy) {
        const unsigned long long* row = kb + (size_t)(py * SS + sy) * S + px * SS;
        if constexpr (SS == 2) {      // S is even and the buffer 256-byte aligned: the two keys of a sample row are one 16-byte load
            const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(row);
            k[sy * SS] = v.x; k[sy * SS + 1] = v.y;
        } else {
            k[sy * SS] = row[0];
        }
    }
    float acc[3] = {0.f, 0.f, 0.f}, zacc = 0.f, aacc = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float c[3] = {bg0, bg1, bg2}, z = far;
        if (k[s] != SP_EMPTY) {
            const size_t i = (size_t)b * N + (unsigned)k[s];
            SplatPoint p;
            sp_load(pts, radius, radius_px, SS, Sf, near, far, i, p);     // true: the point took this sample
            const float d2 = sp_d2(px * SS + (s % SS), py * SS + (s / SS), p.px, p.py);
            const float t = __fsub_rn(1.f, d2 / __fmul_rn(p.rs, p.rs));
            const float shade = __fadd_rn(ambient, __fmul_rn(direct, sqrtf(fmaxf(0.f, t))));
#pragma unroll
            for (int q = 0; q < 3; ++q) c[q] = __fmul_rn(colors ? colors[3 * i + q] : 1.f, shade);
            z = p.z;
            aacc += 1.f;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] += c[q];
        zacc += z;
    }
    constexpr float inv_ns = 1.f / NS;
    const int row = size - 1 - py;                        // the flip of chore_render_fwd
    const size_t plane = (size_t)size * size, o = (size_t)row * size + px;
#pragma unroll
    for (int q = 0; q < 3; ++q) rgb[((size_t)b * 3 + q) * plane + o] = acc[q] * inv_ns;
    depth_out[(size_t)b * plane + o] = zacc * inv_ns;
    alpha_out[(size_t)b * plane + o] = aacc * inv_ns;
    if (sample_point_index) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
            sample_point_index[((size_t)b * S + (py * SS + s / SS)) * S + (px * SS + s % SS)] =
                k[s] == SP_EMPTY ? -1 : (int)(unsigned)k[s];
    }
}

bool splat_shape_ok(int B, int N, int size, int ssaa) {
    return B >= 1 && B <= 65535 && N >= 1 && size >= 1 && (ssaa == 1 || ssaa == 2) && (long long)size * ssaa <= 4096 &&
           (long long)B * N <= 0x7fffffffLL - 256 && (long long)B * size * ssaa * size * ssaa <= (1LL << 31);
}

}  // namespace

extern "C" size_t chore_splat_workspace_bytes(int B, int N, int size, int ssaa) {
    if (!splat_shape_ok(B, N, size, ssaa)) return 0;
    const size_t S = (size_t)size * ssaa;
    return (size_t)B * S * S * sizeof(unsigned long long);
}

extern "C" int chore_splat_fwd(chore_handle* h, const float* pts, const float* rgb_in, const float* radius, float radius_px,
                               int B, int N, int size, int ssaa, float ambient, float near_z, float far_z,
                               const float* background3, float* rgb, float* depth, float* alpha, int* sample_point_index,
                               void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!pts || !background3 || !rgb || !depth || !alpha || !workspace)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_splat_fwd: null argument");
    if (ssaa != 1 && ssaa != 2) CHORE_FAIL(h, CHORE_EINVAL, "chore_splat_fwd: ssaa must be 1 or 2, got %d", ssaa);
    if (!splat_shape_ok(B, N, size, ssaa))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_splat_fwd: bad sizes B=%d N=%d size=%d ssaa=%d", B, N, size, ssaa);
    if (!(ambient >= 0.f && ambient <= 1.f))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_splat_fwd: ambient must lie in [0, 1], got %g", (double)ambient);
    if (!(near_z < far_z))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_splat_fwd: near_z %g must be below far_z %g", (double)near_z, (double)far_z);
    if (!radius && !(radius_px > 0.f))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_splat_fwd: radius_px must be positive without per-point radii, got %g",
                   (double)radius_px);
    hipStream_t s = (hipStream_t)stream;
    const int S = size * ssaa, total = B * N;
    unsigned long long* keys = (unsigned long long*)workspace;
    const size_t nkeys = (size_t)B * S * S;
    hipLaunchKernelGGL(splat_clear_kernel, dim3((unsigned)((nkeys / 2 + 256) / 256)), dim3(256), 0, s, keys, nkeys);
    CHORE_LAUNCH_CHECK(h, s);
    hipLaunchKernelGGL(splat_kernel, dim3((total + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, pts, radius, radius_px, total, N, S, ssaa,
                       near_z, far_z, keys);
    CHORE_LAUNCH_CHECK(h, s);
    const dim3 grid((size + 63) / 64, (size + 3) / 4, B);
    if (ssaa == 2)
        hipLaunchKernelGGL(splat_resolve_kernel<2>, grid, dim3(256), 0, s, keys, pts, rgb_in, radius, radius_px, N, size,
                           ambient, near_z, far_z, background3[0], background3[1], background3[2], rgb, depth, alpha,
                           sample_point_index);
    else
        hipLaunchKernelGGL(splat_resolve_kernel<1>, grid, dim3(256), 0, s, keys, pts, rgb_in, radius, radius_px, N, size,
                           ambient, near_z, far_z, background3[0], background3[1], background3[2], rgb, depth, alpha,
                           sample_point_index);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
