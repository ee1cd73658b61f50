// raster_common.h -- what the silhouette rasteriser (silhouette.hip) and the colour / depth rasteriser (render.hip) share:
// the per-triangle setup and the per-sample hit rule of neural_renderer's forward_face_index_map
// (external/neural_renderer/neural_renderer/cuda/rasterize_cuda_kernel.cu:24-215).  Both kernels evaluate these very
// expressions (explicit __fmul_rn, fixed association, -ffp-contract=off), so the face that wins a sample is the same bit
// for bit in both.
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

// normalised coordinate of the centre of pixel i of `size` (evaluated in double, stored as float, like the reference)
__device__ __forceinline__ float raster_centre(int i, int size) { return (float)((2.0 * i + 1 - size) / size); }

// does the sample (xp, yp) normalised / (xf, yf) pixel hit the front-facing triangle (f, inverse m)?  On a hit: the clamped
// and renormalised barycentric weights and the perspective-correct depth zp, already checked against near / far.
__device__ __forceinline__ bool raster_hit(const float* f, const float* m, float xp, float yp, float xf, float yf, float near,
                                           float far, float* w, float& zp) {
    if (__fmul_rn(yp - f[1], f[3] - f[0]) < __fmul_rn(xp - f[0], f[4] - f[1]) ||
        __fmul_rn(yp - f[4], f[6] - f[3]) < __fmul_rn(xp - f[3], f[7] - f[4]) ||
        __fmul_rn(yp - f[7], f[0] - f[6]) < __fmul_rn(xp - f[6], f[1] - f[7]))
        return false;
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
    return !(zp <= near || far <= zp);
}

}  // namespace
