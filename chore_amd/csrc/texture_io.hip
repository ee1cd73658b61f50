// texture_io.hip -- the texture side of the OBJ file interface: texture cubes from UV triangles and texture images
// (chore_load_textures, neural_renderer's load_textures), and one image with a tile per face from texture cubes
// (chore_texture_atlas, neural_renderer's create_texture_image).  Forward only.
//
// The rules are written out in include/chore_hip.h.  Organisation, as in photo_tex.hip:
//   * one thread per output record (a texel, a pixel: three floats), consecutive threads on consecutive records; the block's 256
//     records go through LDS so that every store instruction of a wave covers 256 contiguous bytes;
//   * no workspace, no atomics, one writer per output element: bit-equal from call to call.  Nothing is written but the output:
//     the UVs are wrapped in registers, and the atlas' diagonal pixels evaluate their left neighbour's formula themselves;
//   * all materials in one launch: the image table (offset, height, width per image) is host data, checked against the size of
//     `images` before the launch and passed by value, so no load can leave `images` whatever the UVs are;
//   * every index into an image or a cube is clamped before it is used.
#include "common.h"

#include <cmath>

namespace {

constexpr int TI_BLOCK = 256;
constexpr int TI_MAX_GRID = 1 << 20;      // blocks; a grid-stride loop covers what lies beyond
constexpr int TI_MAX_IMAGES = 128;        // entries of the by-value image table (2 KB of kernel arguments)
constexpr int TI_MAX_SIDE = 16384;        // pixels per side of an atlas

struct TiImage {
    long long off;      // of pixel (0,0) in `images`, bytes
    int H, W;
};
struct TiImageTable {
    TiImage e[TI_MAX_IMAGES];
};

// step 4: the reference's mod, fp32
__device__ __forceinline__ float ti_mod(float x, float y) { return x > 0.f ? fmodf(x, y) : y + fmodf(x, y); }

__device__ __forceinline__ float ti_wrap(float x, int wrapping) {
    if (wrapping == 0) return ti_mod(x, 1.0f);
    if (wrapping == 1) return ti_mod(x, 2.0f) < 1.0f ? ti_mod(x, 1.0f) : 1.0f - ti_mod(x, 1.0f);
    return fminf(fmaxf(x, 0.0f), 1.0f);
}

// pixel (row r of the flipped image, column x), channel ch, both already inside the image
__device__ __forceinline__ float ti_pixel(const unsigned char* __restrict__ img, int H, int W, int r, int x, int ch) {
    return (float)img[((size_t)(H - 1 - r) * W + x) * 3 + ch] / 255.0f;
}

// the block's records, staged as 3 * TI_BLOCK floats, to out[base * 3 ...): contiguous per store instruction
__device__ __forceinline__ void ti_flush(const float* stage, float* __restrict__ out, size_t base, size_t total) {
    const size_t left = total - base;
    const int nfl = left < (size_t)TI_BLOCK ? (int)left * 3 : TI_BLOCK * 3;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int o = q * TI_BLOCK + threadIdx.x;
        if (o < nfl) out[base * 3 + o] = stage[o];
    }
}

// thread = texel, x fastest over (k, j, i, f): the order of `textures`
__global__ __launch_bounds__(TI_BLOCK) void load_textures_kernel(const float* __restrict__ uv, const int* __restrict__ face_image,
                                                                 const float* __restrict__ face_color,
                                                                 const unsigned char* __restrict__ images, const TiImageTable tab,
                                                                 int M, size_t total, int ts, int wrapping, int bilinear,
                                                                 float* __restrict__ textures) {
    __shared__ float stage[TI_BLOCK * 3];
    const int ts3 = ts * ts * ts;
    const size_t nblk = (total + TI_BLOCK - 1) / TI_BLOCK;
    for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const size_t base = blk * TI_BLOCK, t = base + threadIdx.x;
        if (t < total) {
            const size_t f = t / (size_t)ts3;
            const int local = (int)(t - f * (size_t)ts3);
            const int i = local / (ts * ts), j = (local / ts) % ts, k = local % ts;
            const float* fc = face_color + f * 3;
            float c[3] = {fc[0], fc[1], fc[2]};                                   // 1. colour-only faces, and the fallback
            const int m = face_image[f];
            if (m >= 0 && m < M) {
                const float* u6 = uv + f * 6;
                float w[6];
                bool finite = true;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    w[q] = u6[q];
                    finite = finite && isfinite(w[q]);
                }
                if (wrapping == 3) {                                              // 2. CLAMP_TO_BORDER: zeros, never sampled
                    c[0] = c[1] = c[2] = 0.0f;
                } else if (finite) {
                    // 3. weights
                    const float tf = (float)(ts - 1);
                    float d0 = (float)i / tf, d1 = (float)j / tf, d2 = (float)k / tf;
                    const float s = (d0 + d1) + d2;
                    if (s > 0.0f) {
                        d0 /= s; d1 /= s; d2 /= s;
                    }
                    // 4. wrap, in registers
#pragma unroll
                    for (int q = 0; q < 6; ++q) w[q] = ti_wrap(w[q], wrapping);
                    // 5. position in the flipped image
                    const int H = tab.e[m].H, W = tab.e[m].W;
                    const unsigned char* img = images + tab.e[m].off;
                    const float px = ((w[0] * d0 + w[2] * d1) + w[4] * d2) * (float)(W - 1);
                    const float py = ((w[1] * d0 + w[3] * d1) + w[5] * d2) * (float)(H - 1);
                    // 6. sample; every index clamped into the image
                    if (bilinear) {
                        const int xi = (int)px, yi = (int)py;
                        const float fx = px - (float)xi, fy = py - (float)yi;
                        const int x0 = min(max(xi, 0), W - 1), y0 = min(max(yi, 0), H - 1);
                        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            const float a = ti_pixel(img, H, W, y0, x0, ch), b = ti_pixel(img, H, W, y1, x0, ch);
                            const float top = a + (ti_pixel(img, H, W, y0, x1, ch) - a) * fx;      // equal taps give their value exactly
                            const float bot = b + (ti_pixel(img, H, W, y1, x1, ch) - b) * fx;
                            c[ch] = top + (bot - top) * fy;
                        }
                    } else {
                        const int x0 = min(max((int)roundf(px), 0), W - 1), y0 = min(max((int)roundf(py), 0), H - 1);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) c[ch] = ti_pixel(img, H, W, y0, x0, ch);
                    }
                }
            }
            stage[3 * threadIdx.x + 0] = c[0];
            stage[3 * threadIdx.x + 1] = c[1];
            stage[3 * threadIdx.x + 2] = c[2];
        }
        __syncthreads();
        ti_flush(stage, textures, base, total);
        __syncthreads();
    }
}

// thread = pixel of the file's image, x fastest: the order of `image`
__global__ __launch_bounds__(TI_BLOCK) void texture_atlas_kernel(const float* __restrict__ textures, size_t total, int F, int tsi,
                                                                 int tso, int tile_w, int Hh, int Ww, float* __restrict__ image) {
    __shared__ float stage[TI_BLOCK * 3];
    const size_t nblk = (total + TI_BLOCK - 1) / TI_BLOCK;
    const float eps = 1e-5f;
    for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const size_t base = blk * TI_BLOCK, t = base + threadIdx.x;
        if (t < total) {
            const int r = (int)(t / (size_t)Ww), x = (int)(t - (size_t)r * Ww);
            const int y = Hh - 1 - r;                                             // counted from the bottom of the file's image
            // 1. tile and position in it
            const int col = x / tso, row = y / tso;
            const long long fn = (long long)col + (long long)row * tile_w;
            int lx = x % tso;
            const int ly = y % tso, T = tso - 1;
            float c[3] = {0.0f, 0.0f, 0.0f};                                      // 2. a tile without a face
            if (fn < (long long)F) {
                if (ly + 1 == lx) lx -= 1;                                        // 3. the diagonal's right neighbour
                // 4. weights of the tile triangle, tile-local
                const float Tf = (float)T, den = 1.0f + eps;
                const float w[3] = {((float)(T - ly) / Tf) / den, ((float)(ly - lx) / Tf) / den, ((float)lx / Tf) / den};
                // 5. position in the cube
                int lo[3], hi[3];
                float fr[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float tq = fminf(fmaxf(w[q] * (float)(tsi - 1), 0.0f), (float)(tsi - 1) - eps);
                    const int iq = min(max((int)tq, 0), tsi - 1);
                    lo[q] = iq;
                    hi[q] = min(iq + 1, tsi - 1);
                    fr[q] = tq - (float)iq;
                }
                const float* cube = textures + (size_t)fn * tsi * tsi * tsi * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float plane[2];
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        const int ia = a ? hi[0] : lo[0];
                        float line[2];
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const int jb = b ? hi[1] : lo[1];
                            const float* p = cube + ((size_t)(ia * tsi + jb) * tsi) * 3 + ch;
                            const float v0 = p[lo[2] * 3];
                            line[b] = v0 + (p[hi[2] * 3] - v0) * fr[2];
                        }
                        plane[a] = line[0] + (line[1] - line[0]) * fr[1];
                    }
                    c[ch] = plane[0] + (plane[1] - plane[0]) * fr[0];
                }
            }
            stage[3 * threadIdx.x + 0] = c[0];
            stage[3 * threadIdx.x + 1] = c[1];
            stage[3 * threadIdx.x + 2] = c[2];
        }
        __syncthreads();
        ti_flush(stage, image, base, total);
        __syncthreads();
    }
}

inline int ti_grid(size_t total) {
    const size_t nblk = (total + TI_BLOCK - 1) / TI_BLOCK;
    return (int)(nblk < (size_t)TI_MAX_GRID ? nblk : (size_t)TI_MAX_GRID);
}

// tile counts in integer arithmetic; false where a side exceeds TI_MAX_SIDE
inline bool ti_atlas_tiles(int F, int tso, int* tile_w, int* tile_h) {
    if (F < 1 || tso < 2 || tso > TI_MAX_SIDE) return false;
    long long rt = (long long)std::sqrt((double)(F - 1));
    while (rt * rt > (long long)(F - 1)) --rt;
    while ((rt + 1) * (rt + 1) <= (long long)(F - 1)) ++rt;
    const long long tw = rt + 1, th = (long long)(F - 1) / tw + 1;
    if (tw * tso > TI_MAX_SIDE || th * tso > TI_MAX_SIDE) return false;
    *tile_w = (int)tw;
    *tile_h = (int)th;
    return true;
}

}  // namespace

extern "C" int chore_load_textures(chore_handle* h, const float* uv, const int* face_image, const float* face_color,
                                   const unsigned char* images, size_t images_bytes, const long long* image_off,
                                   const int* image_hw, int M, int F, int ts, int wrapping, int bilinear, float* textures,
                                   chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!uv || !face_image || !face_color || !textures) CHORE_FAIL(h, CHORE_EINVAL, "chore_load_textures: null argument");
    if (F < 1 || ts < 2 || ts > 16 || M < 0 || M > TI_MAX_IMAGES)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_load_textures: bad sizes F=%d ts=%d M=%d", F, ts, M);
    if (wrapping < 0 || wrapping > 3) CHORE_FAIL(h, CHORE_EINVAL, "chore_load_textures: unknown wrapping mode %d", wrapping);
    if (M > 0 && (!images || !image_off || !image_hw)) CHORE_FAIL(h, CHORE_EINVAL, "chore_load_textures: null image table");
    TiImageTable tab;
    for (int m = 0; m < TI_MAX_IMAGES; ++m) tab.e[m] = TiImage{0, 1, 1};
    for (int m = 0; m < M; ++m) {
        const int H = image_hw[2 * m], W = image_hw[2 * m + 1];
        const long long off = image_off[m];
        if (H < 1 || W < 1) CHORE_FAIL(h, CHORE_EINVAL, "chore_load_textures: image %d is %d x %d", m, H, W);
        const size_t bytes = (size_t)H * (size_t)W * 3;
        if (off < 0 || (size_t)off > images_bytes || bytes > images_bytes - (size_t)off)
            CHORE_FAIL(h, CHORE_EINVAL, "chore_load_textures: image %d (%d x %d at byte %lld) leaves the %zu bytes of images", m, H,
                       W, off, images_bytes);
        tab.e[m] = TiImage{off, H, W};
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)F * ts * ts * ts;
    hipLaunchKernelGGL(load_textures_kernel, dim3(ti_grid(total)), dim3(TI_BLOCK), 0, s, uv, face_image, face_color, images, tab, M,
                       total, ts, wrapping, bilinear, textures);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" int chore_texture_atlas_size(int F, int tso, int* height, int* width) {
    int tw, th;
    if (!height || !width || !ti_atlas_tiles(F, tso, &tw, &th)) return CHORE_EINVAL;
    *height = th * tso;
    *width = tw * tso;
    return CHORE_OK;
}

extern "C" int chore_texture_atlas(chore_handle* h, const float* textures, int F, int tsi, int tso, float* image,
                                   chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!textures || !image) CHORE_FAIL(h, CHORE_EINVAL, "chore_texture_atlas: null argument");
    if (F < 1 || tsi < 2 || tsi > 16 || tso < 2)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_texture_atlas: bad sizes F=%d tsi=%d tso=%d", F, tsi, tso);
    int tw, th;
    if (!ti_atlas_tiles(F, tso, &tw, &th))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_texture_atlas: F=%d tiles of %d px exceed %d px on a side", F, tso, TI_MAX_SIDE);
    hipStream_t s = (hipStream_t)stream;
    const int Hh = th * tso, Ww = tw * tso;
    const size_t total = (size_t)Hh * Ww;
    hipLaunchKernelGGL(texture_atlas_kernel, dim3(ti_grid(total)), dim3(TI_BLOCK), 0, s, textures, total, F, tsi, tso, tw, Hh, Ww,
                       image);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
