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
// The point helpers, splat_kernel, the key loads and the disc shading live in splat_common.h, which scene.hip compiles too.
#include "splat_common.h"

namespace {

// every key = SP_EMPTY.  A kernel, not hipMemsetAsync: the call is recorded into hipGraphs, where byte-memset nodes replay
// unreliably (GPU memory faults; contact.hip fills its workspace with a kernel for the same reason).  16-byte stores; n keys.
__global__ __launch_bounds__(256) void splat_clear_kernel(unsigned long long* __restrict__ keys, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (2 * i + 1 < n)
        reinterpret_cast<ulonglong2*>(keys)[i] = make_ulonglong2(SP_EMPTY, SP_EMPTY);
    else if (2 * i < n)
        keys[2 * i] = SP_EMPTY;
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
    sp_load_keys<SS>(kb, S, px, py, k);
    float acc[3] = {0.f, 0.f, 0.f}, zacc = 0.f, aacc = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float c[3] = {bg0, bg1, bg2}, z = far;
        if (k[s] != SP_EMPTY) {
            const size_t i = (size_t)b * N + (unsigned)k[s];
            sp_shade(pts, colors, radius, radius_px, SS, Sf, near, far, i, px * SS + (s % SS), py * SS + (s / SS), ambient, direct, c, z);
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

}  // namespace

extern "C" size_t chore_splat_workspace_bytes(int B, int N, int size, int ssaa) {
    if (!splat_shape_ok(B, N, size, ssaa)) return 0;
    return splat_key_bytes(B, size, ssaa);
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
