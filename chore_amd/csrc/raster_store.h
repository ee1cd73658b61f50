// raster_store.h -- what every rasteriser of the family does before its first pass and after its last, once: the clear kernel
// (splat.hip, scene.hip, instances.hip), the resolve store and the sample-id store of an output pixel (render.hip, splat.hip,
// scene.hip, instances.hip), and the host's step from `ssaa` to a compile-time SS.  Included by render_common.h and
// splat_common.h; it knows neither triangles nor points.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr unsigned long long SP_EMPTY = ~0ull;       // a sample key no point has taken (splat_common.h)

// keys[0, nkeys) = SP_EMPTY (16-byte stores where a pair is whole) and up to three int ranges = 0, in one grid; an absent range
// has length 0.  A kernel, not hipMemsetAsync: the calls are recorded into hipGraphs, where byte-memset nodes replay unreliably
// (GPU memory faults; contact.hip fills its workspace with a kernel for the same reason).  A thread clears two keys and one int
// of each range.
__global__ __launch_bounds__(256) void raster_clear_kernel(unsigned long long* __restrict__ keys, size_t nkeys, int* __restrict__ a,
                                                           size_t na, int* __restrict__ b, size_t nb, int* __restrict__ c, size_t nc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (2 * i + 1 < nkeys)
        reinterpret_cast<ulonglong2*>(keys)[i] = make_ulonglong2(SP_EMPTY, SP_EMPTY);
    else if (2 * i < nkeys)
        keys[2 * i] = SP_EMPTY;
    if (i < na) a[i] = 0;
    if (i < nb) b[i] = 0;
    if (i < nc) c[i] = 0;
}
// its launch with at least `threads` threads (the caller's: the largest of (nkeys + 1) / 2 and the int ranges)
inline void raster_clear(hipStream_t s, size_t threads, unsigned long long* keys, size_t nkeys, int* a = nullptr, size_t na = 0,
                         int* b = nullptr, size_t nb = 0, int* c = nullptr, size_t nc = 0) {
    hipLaunchKernelGGL(raster_clear_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, keys, nkeys, a, na, b, nb, c, nc);
}

// The resolve of output pixel (px, py) (rows not flipped) of image b: the sums over its NS samples times 1 / NS (rgb, depth and
// alpha alike, like F.avg_pool2d), to the flipped row (rasterize_rgbad flips the rows), channel-first.
template <int NS>
__device__ __forceinline__ void raster_store_resolved(int b, int px, int py, int size, const float* acc, float zacc, float aacc,
                                                      float* __restrict__ rgb, float* __restrict__ depth_out,
                                                      float* __restrict__ alpha_out) {
    constexpr float inv_ns = 1.f / NS;
    const int row = size - 1 - py;
    const size_t plane = (size_t)size * size, o = (size_t)row * size + px;
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[((size_t)b * 3 + k) * plane + o] = acc[k] * inv_ns;
    depth_out[(size_t)b * plane + o] = zacc * inv_ns;
    alpha_out[(size_t)b * plane + o] = aacc * inv_ns;
}

// the ids of the SS x SS samples of output pixel (px, py), id[sy * SS + sx], to the (B, S, S) sample image (rows not flipped)
template <int SS>
__device__ __forceinline__ void raster_store_sample_ids(int* __restrict__ out, int b, int px, int py, int size,
                                                        const int (&id)[SS * SS]) {
    const int S = size * SS;
#pragma unroll
    for (int sy = 0; sy < SS; ++sy)
#pragma unroll
        for (int sx = 0; sx < SS; ++sx) out[((size_t)b * S + (py * SS + sy)) * S + (px * SS + sx)] = id[sy * SS + sx];
}

// fn(std::integral_constant<int, SS>) for ssaa = SS in {1, 2} (checked by the caller): the tile kernels take SS at compile time
template <class Fn>
inline void raster_dispatch_ssaa(int ssaa, Fn&& fn) {
    if (ssaa == 2) fn(std::integral_constant<int, 2>{});
    else fn(std::integral_constant<int, 1>{});
}

}  // namespace
