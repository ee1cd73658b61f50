// splat_common.h -- what the point rasteriser (splat.hip) and the scene rasteriser (scene.hip) share: the point helpers, the
// point pass that fills the 64-bit sample keys with its launch, the disc shading of a sample's winner, and the checks of the
// point arguments under the caller's name.  Both files compile these very
// expressions (explicit __fmul_rn / __fadd_rn / __fsub_rn, fixed association, -ffp-contract=off), so the point that wins a
// sample and its shaded colour are the same bit for bit in both.
#pragma once
#include "raster_store.h"     // SP_EMPTY, the clear kernel, the resolve and id stores

namespace {

constexpr float SP_MAX_RS = 64.f;    // radii are clamped to this many samples
constexpr float SP_LANE_RS = 2.f;    // up to here a disc is drawn by the lane that loaded it

// sample-space position of a normalised coordinate: raster_common.h's vertex expression, 0.5f * ((u * S + S) - 1.0f)
__device__ __forceinline__ float sp_pos(float u, float Sf) {
    return __fmul_rn(0.5f, __fsub_rn(__fadd_rn(__fmul_rn(u, Sf), Sf), 1.0f));
}

struct SplatPoint {
    float px, py, z, rs;
};

// point i of the flattened (B*N) list; false = skipped (NaN, radius <= 0, outside the depth range).  chore_amd.render.rasterize_scene
// relies on `far <= z` being skipped: without points but with a face_opacity it passes one point at z == far that must never draw.
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

// the winner of sample (xi, yj) of image b, index n taken from its key: the colour times the sphere shade, and the depth.
// d2 is recomputed with the very expressions of the coverage test.
__device__ __forceinline__ void sp_shade(const float* __restrict__ pts, const float* __restrict__ colors,
                                         const float* __restrict__ radius, float radius_px, int SS, float Sf, float near,
                                         float far, size_t i, int xi, int yj, float ambient, float direct, float* c, float& z) {
    SplatPoint p;
    sp_load(pts, radius, radius_px, SS, Sf, near, far, i, p);     // true: the point took this sample
    const float d2 = sp_d2(xi, yj, p.px, p.py);
    const float t = __fsub_rn(1.f, d2 / __fmul_rn(p.rs, p.rs));
    const float shade = __fadd_rn(ambient, __fmul_rn(direct, sqrtf(fmaxf(0.f, t))));
#pragma unroll
    for (int q = 0; q < 3; ++q) c[q] = __fmul_rn(colors ? colors[3 * i + q] : 1.f, shade);
    z = p.z;
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

// the SS x SS keys of output pixel (px, py), k[sy * SS + sx]; kb = the image's keys, S = size * SS
template <int SS>
__device__ __forceinline__ void sp_load_keys(const unsigned long long* __restrict__ kb, int S, int px, int py,
                                             unsigned long long* k) {
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
}

inline bool splat_shape_ok(int B, int N, int size, int ssaa) {
    return B >= 1 && B <= 65535 && N >= 1 && size >= 1 && (ssaa == 1 || ssaa == 2) && (long long)size * ssaa <= 4096 &&
           (long long)B * N <= 0x7fffffffLL - 256 && (long long)B * size * ssaa * size * ssaa <= (1LL << 31);
}
inline size_t splat_key_bytes(int B, int size, int ssaa) {
    const size_t S = (size_t)size * ssaa;
    return (size_t)B * S * S * sizeof(unsigned long long);
}
// the checks of the point arguments that chore_splat_fwd and the scene entry points share, under the caller's name
inline int sp_check_args(chore_handle* h, const char* who, float ambient, float near_z, float far_z, const float* radius,
                         float radius_px) {
    if (!(ambient >= 0.f && ambient <= 1.f))
        CHORE_FAIL(h, CHORE_EINVAL, "%s: ambient must lie in [0, 1], got %g", who, (double)ambient);
    if (!(near_z < far_z))
        CHORE_FAIL(h, CHORE_EINVAL, "%s: near_z %g must be below far_z %g", who, (double)near_z, (double)far_z);
    if (!radius && !(radius_px > 0.f))
        CHORE_FAIL(h, CHORE_EINVAL, "%s: radius_px must be positive without per-point radii, got %g", who, (double)radius_px);
    return CHORE_OK;
}
// the point pass on stream s: every sample key of the (B, S, S) grid, cleared before, takes its nearest point
inline void splat_pass(hipStream_t s, const float* pts, const float* radius, float radius_px, int B, int N, int S, int ssaa,
                       float near_z, float far_z, unsigned long long* keys) {
    const int total = B * N;
    hipLaunchKernelGGL(splat_kernel, dim3((total + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, pts, radius, radius_px, total, N, S,
                       ssaa, near_z, far_z, keys);
}

}  // namespace
