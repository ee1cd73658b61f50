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
// This file holds the resolve kernel and the entry point.  The point helpers, splat_kernel with its launch, the key loads, the
// disc shading and the argument checks live in splat_common.h, which scene.hip compiles too; the clear kernel (keys = empty; why
// it is a kernel is said there), the resolve and id stores and the ssaa dispatch in raster_store.h.
#include "splat_common.h"

namespace {

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
    int id[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float c[3] = {bg0, bg1, bg2}, z = far;
        id[s] = k[s] == SP_EMPTY ? -1 : (int)(unsigned)k[s];
        if (k[s] != SP_EMPTY) {
            const size_t i = (size_t)b * N + (unsigned)k[s];
            sp_shade(pts, colors, radius, radius_px, SS, Sf, near, far, i, px * SS + (s % SS), py * SS + (s / SS), ambient, direct, c, z);
            aacc += 1.f;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] += c[q];
        zacc += z;
    }
    raster_store_resolved<NS>(b, px, py, size, acc, zacc, aacc, rgb, depth_out, alpha_out);      // chore_render_fwd's resolve
    if (sample_point_index) raster_store_sample_ids<SS>(sample_point_index, b, px, py, size, id);
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
    if (int rc = sp_check_args(h, "chore_splat_fwd", ambient, near_z, far_z, radius, radius_px)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int S = size * ssaa;
    unsigned long long* keys = (unsigned long long*)workspace;
    const size_t nkeys = (size_t)B * S * S;
    raster_clear(s, nkeys / 2 + 1, keys, nkeys);
    CHORE_LAUNCH_CHECK(h, s);
    splat_pass(s, pts, radius, radius_px, B, N, S, ssaa, near_z, far_z, keys);
    CHORE_LAUNCH_CHECK(h, s);
    raster_dispatch_ssaa(ssaa, [&](auto ss) {
        hipLaunchKernelGGL(splat_resolve_kernel<decltype(ss)::value>, dim3((size + 63) / 64, (size + 3) / 4, B), dim3(256), 0, s, keys,
                           pts, rgb_in, radius, radius_px, N, size, ambient, near_z, far_z, background3[0], background3[1],
                           background3[2], rgb, depth, alpha, sample_point_index);
    });
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
