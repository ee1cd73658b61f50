// photo_tex.hip -- photo textures and point visibility: colour the texture cube of every face from the photo the fit was made
// from, at the texels the camera sees, and say whether a projected point is seen.  Forward only.
//
// The rule is chore_photo_textures_fwd's in include/chore_hip.h.  Organisation:
//   * pt_seen is the visibility rule (depth range, nearest sample, depth test against the depth image) and the only place it is
//     written: the texel kernel calls it on the texel's (u, v, z), the point kernel on the point's.  A texel whose weights are
//     one-hot lands on its vertex bit for bit, so both kernels agree there exactly.
//   * one thread per texel, consecutive threads on consecutive texels: at ts = 4 a wave is one face and its nine vertex floats and
//     three fallback floats are broadcast loads.  The kernel is write-bound (12 bytes per texel); the block's 256 colours go
//     through LDS so that every store instruction of a wave covers 256 contiguous bytes instead of 64 strided 12-byte records.
//   * no workspace, no atomics: every output element has one writer, so the result is bit-equal from call to call.
#include "common.h"

namespace {

constexpr int PT_BLOCK = 256;
constexpr int PT_MAX_GRID = 1 << 20;      // blocks; a grid-stride loop covers what lies beyond
constexpr int PT_MAX_DIM = 4096;          // the rasterisers' limit on a sample grid

// steps 2, 4 and 5: is the projected position (u, v) at depth z seen in the S x S depth image `dimg` (rows not flipped)?
__device__ __forceinline__ bool pt_seen(float u, float v, float z, const float* __restrict__ dimg, int S, float near, float far,
                                        float bias) {
    if (!(near < z && z < far)) return false;
    const float Sf = (float)S;
    const float px = 0.5f * ((u * Sf + Sf) - 1.0f), py = 0.5f * ((v * Sf + Sf) - 1.0f);
    const float xf = floorf(px + 0.5f), yf = floorf(py + 0.5f);
    if (!(xf >= 0.f && xf <= (float)(S - 1) && yf >= 0.f && yf <= (float)(S - 1))) return false;      // NaN falls here
    return z <= dimg[(size_t)(int)yf * S + (int)xf] + bias;
}

// step 6: the photo position of (u, v); true iff it lies in the Hp x Wp photo
__device__ __forceinline__ bool pt_photo_pos(float u, float v, int Hp, int Wp, int align_corners, float& qx, float& qy) {
    const float Wf = (float)Wp;
    if (align_corners) {
        qx = ((u + 1.0f) * 0.5f) * (Wf - 1.0f);
        qy = ((1.0f - v) * 0.5f) * (Wf - 1.0f);
    } else {
        qx = 0.5f * ((u * Wf + Wf) - 1.0f);
        qy = 0.5f * (((-v) * Wf + Wf) - 1.0f);
    }
    return -0.5f <= qx && qx <= Wf - 0.5f && -0.5f <= qy && qy <= (float)Hp - 0.5f;
}

// the bilinear blend of the four taps around (qx, qy) of the three planes of `photo`, tap indices clamped to the photo
__device__ __forceinline__ void pt_photo_blend(const float* __restrict__ photo, int Hp, int Wp, float qx, float qy, float* c) {
    const float x0f = floorf(qx), y0f = floorf(qy);
    const float fx = qx - x0f, fy = qy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int xa = min(max(x0, 0), Wp - 1), xb = min(max(x0 + 1, 0), Wp - 1);
    const int ya = min(max(y0, 0), Hp - 1), yb = min(max(y0 + 1, 0), Hp - 1);
    const size_t plane = (size_t)Hp * Wp;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* p = photo + ch * plane;
        const float a = p[(size_t)ya * Wp + xa], bq = p[(size_t)yb * Wp + xa];
        const float top = a + (p[(size_t)ya * Wp + xb] - a) * fx;       // equal taps give their value exactly
        const float bot = bq + (p[(size_t)yb * Wp + xb] - bq) * fx;
        c[ch] = top + (bot - top) * fy;
    }
}

// thread = texel, x fastest over (k, j, i, f, b): the order of `textures`
__global__ __launch_bounds__(PT_BLOCK) void photo_textures_kernel(const float* __restrict__ tri, const float* __restrict__ depth,
                                                                  const float* __restrict__ photo, const float* __restrict__ fallback,
                                                                  size_t total, int F, int ts, int S, int Hp, int Wp, float near,
                                                                  float far, float bias, int align_corners,
                                                                  float* __restrict__ textures, unsigned char* __restrict__ seen_out) {
    __shared__ float stage[PT_BLOCK * 3];
    const int ts3 = ts * ts * ts;
    const size_t nblk = (total + PT_BLOCK - 1) / PT_BLOCK;
    for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const size_t base = blk * PT_BLOCK, t = base + threadIdx.x;
        if (t < total) {
            const size_t face = t / (size_t)ts3;              // b * F + f
            const int local = (int)(t - face * (size_t)ts3);
            const int i = local / (ts * ts), j = (local / ts) % ts, k = local % ts;
            const size_t b = face / (size_t)F;
            const float* f9 = tri + face * 9;
            const float* fb = fallback + face * 3;
            float c[3] = {fb[0], fb[1], fb[2]};
            // 1. weights
            const int n = i + j + k;
            float w0 = 1.0f / 3.0f, w1 = 1.0f / 3.0f, w2 = 1.0f / 3.0f;
            if (n > 0) {
                const float nf = (float)n;
                w0 = (float)i / nf; w1 = (float)j / nf; w2 = (float)k / nf;
            }
            // 2. depth, 3. screen position
            const float z0 = f9[2], z1 = f9[5], z2 = f9[8];
            const float z = (w0 * z0 + w1 * z1) + w2 * z2;
            const float s0 = (w0 * z0) / z, s1 = (w1 * z1) / z, s2 = (w2 * z2) / z;
            const float u = (s0 * f9[0] + s1 * f9[3]) + s2 * f9[6];
            const float v = (s0 * f9[1] + s1 * f9[4]) + s2 * f9[7];
            // 2, 4, 5. visibility
            const bool seen = pt_seen(u, v, z, depth + b * (size_t)S * S, S, near, far, bias);
            // 6. photo lookup
            float qx, qy;
            if (seen && pt_photo_pos(u, v, Hp, Wp, align_corners, qx, qy))
                pt_photo_blend(photo + b * 3 * (size_t)Hp * Wp, Hp, Wp, qx, qy, c);
            if (seen_out) seen_out[t] = seen ? 1 : 0;
            stage[3 * threadIdx.x + 0] = c[0];
            stage[3 * threadIdx.x + 1] = c[1];
            stage[3 * threadIdx.x + 2] = c[2];
        }
        __syncthreads();
        // 7. the block's 768 floats, contiguous in `textures`
        const size_t left = total - base;
        const int nfl = left < (size_t)PT_BLOCK ? (int)left * 3 : PT_BLOCK * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int o = q * PT_BLOCK + threadIdx.x;
            if (o < nfl) textures[base * 3 + o] = stage[o];
        }
        __syncthreads();
    }
}

// thread = point
__global__ __launch_bounds__(PT_BLOCK) void point_visibility_kernel(const float* __restrict__ pts, const float* __restrict__ depth,
                                                                    size_t total, int N, int S, float near, float far, float bias,
                                                                    int* __restrict__ visible) {
    for (size_t t = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x; t < total; t += (size_t)gridDim.x * PT_BLOCK) {
        const size_t b = t / (size_t)N;
        const float* p = pts + t * 3;
        visible[t] = pt_seen(p[0], p[1], p[2], depth + b * (size_t)S * S, S, near, far, bias) ? 1 : 0;
    }
}

inline int pt_grid(size_t total) {
    const size_t nblk = (total + PT_BLOCK - 1) / PT_BLOCK;
    return (int)(nblk < (size_t)PT_MAX_GRID ? nblk : (size_t)PT_MAX_GRID);
}

}  // namespace

extern "C" int chore_photo_textures_fwd(chore_handle* h, const float* tri, const float* depth, const float* photo,
                                        const float* fallback, int B, int F, int ts, int S, int Hp, int Wp, float near_z,
                                        float far_z, float depth_bias, int align_corners, float* textures,
                                        unsigned char* texel_visible, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!tri || !depth || !photo || !fallback || !textures)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_photo_textures_fwd: null argument");
    if (B < 1 || F < 1 || ts < 2 || ts > 16 || S < 1 || S > PT_MAX_DIM)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_photo_textures_fwd: bad sizes B=%d F=%d ts=%d S=%d", B, F, ts, S);
    if (Hp < 1 || Wp < 1 || Hp > Wp)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_photo_textures_fwd: photo of %d rows in a square of side %d", Hp, Wp);
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)B * F * ts * ts * ts;
    hipLaunchKernelGGL(photo_textures_kernel, dim3(pt_grid(total)), dim3(PT_BLOCK), 0, s, tri, depth, photo, fallback, total, F, ts,
                       S, Hp, Wp, near_z, far_z, depth_bias, align_corners, textures, texel_visible);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" int chore_point_visibility(chore_handle* h, const float* pts, const float* depth, int B, int N, int S, float near_z,
                                      float far_z, float depth_bias, int* visible, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!pts || !depth || !visible) CHORE_FAIL(h, CHORE_EINVAL, "chore_point_visibility: null argument");
    if (B < 1 || N < 1 || S < 1 || S > PT_MAX_DIM)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_point_visibility: bad sizes B=%d N=%d S=%d", B, N, S);
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)B * N;
    hipLaunchKernelGGL(point_visibility_kernel, dim3(pt_grid(total)), dim3(PT_BLOCK), 0, s, pts, depth, total, N, S, near_z, far_z,
                       depth_bias, visible);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
