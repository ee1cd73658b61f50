// image_prep.hip -- the image preparation of the test loader on the device, and of the training loader
// (BehaveDataset.prepare_image_crop data/train_data.py:134-149: PIL's Gaussian blur, the mirror, the batched crop / compose).
// (use_mean_center=True, the COCO loader: the float64 canvas of pad_image test_data.py:133-160 and cv2's generic float
// resize -- see prep_compose_mean_kernel below.)
//
// Replaces, from the decoded uint8 images on, TestData.prepare_image_crop (/root/reference/data/test_data.py:59-125,
// use_mean_center=False) = BaseDataset.masks2bbox (data/base_data.py:92-112) + cv2.resize to the 2048-px space (:82-84)
// + BaseDataset.crop (:131-162) + BaseDataset.resize to the network input (:164-176) + compose_images (:178-192).
// The arithmetic is integer: cv2's 8-bit INTER_LINEAR path (11-bit coefficients, see oracle/image_prep.py for the
// restated algorithm -- PARITY UNPINNED at cv2, which is not in this image) -- and the results are bit-identical to the
// oracle.  HBM-bound byte work: one thread per output pixel, coalesced along x, nothing staged.
#include "common.h"

namespace {

constexpr int COEF_BITS = 11;

// source index and 11-bit weights of destination index d for a resize n_src -> n_dst (cv2 resize.cpp, linear, 8U)
__device__ __forceinline__ void lin_coef(int d, int n_src, int n_dst, bool clamp_weights, int& s, int& c0, int& c1) {
    const double scale = (double)n_src / (double)n_dst;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f = f - (float)s;
    if (clamp_weights) {                       // columns: the weight moves to the inner sample at the borders
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    }
    c0 = (int)rintf((1.0f - f) * 2048.0f);
    c1 = (int)rintf(f * 2048.0f);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct Src {                                   // a (h, w, C) uint8 image seen through the crop of base_data.py:131-162
    const unsigned char* p;
    int h, w, C;
    // crop: virtual image of size (ch, cw); column c maps to source column x1 + (c - p1) when p1 <= c < p1 + nx, else 0
    int x1, y1, nx, ny, p1, p2;
    int flip;                                  // the crop is taken from the horizontal mirror: column x reads column w - 1 - x
    __device__ __forceinline__ int at(int y, int x, int k) const {
        const int sx = x - p1, sy = y - p2;
        if (sx < 0 || sx >= nx || sy < 0 || sy >= ny) return 0;
        const int xs = flip ? w - 1 - (x1 + sx) : x1 + sx;
        return p[((size_t)(y1 + sy) * w + xs) * C + k];
    }
};

// one resized sample (cv2 fixed point) of channel k at destination (dy, dx) of a (ch, cw) -> (dh, dw) resize
__device__ __forceinline__ int resize_sample(const Src& s, int ch, int cw, int dh, int dw, int dy, int dx, int k) {
    if (cw == dw && ch == dh) return s.at(dy, dx, k);
    if (cw == 2 * dw && ch == 2 * dh)          // INTER_LINEAR takes the INTER_AREA fast path for an exact 2 x 2 downscale
        return (s.at(2 * dy, 2 * dx, k) + s.at(2 * dy, 2 * dx + 1, k) + s.at(2 * dy + 1, 2 * dx, k) + s.at(2 * dy + 1, 2 * dx + 1, k) + 2) >> 2;
    int sx, a0, a1, sy, b0, b1;
    lin_coef(dx, cw, dw, true, sx, a0, a1);
    lin_coef(dy, ch, dh, false, sy, b0, b1);
    const int sx1 = min(sx + 1, cw - 1);
    const int y0 = clampi(sy, 0, ch - 1), y1 = clampi(sy + 1, 0, ch - 1);
    const int r0 = s.at(y0, sx, k) * a0 + s.at(y0, sx1, k) * a1;
    const int r1 = s.at(y1, sx, k) * a0 + s.at(y1, sx1, k) * a1;
    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    return clampi(v, 0, 255);
}

__global__ void prep_bbox_kernel(const unsigned char* m0, const unsigned char* m1, int H, int W, int thres, int* out4) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    bool fg = false;
    if (x < W) {
        const size_t o = (size_t)y * W + x;
        const unsigned char sum = (unsigned char)(m0[o] + (m1 ? m1[o] : 0));      // uint8 wrap-around like numpy's +=
        fg = sum > thres;
    }
    // one atomic per wave and bound
    int xmin = fg ? x : 0x7fffffff, xmax = fg ? x + 1 : -0x7fffffff;
    for (int o = 32; o; o >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, o));
        xmax = max(xmax, __shfl_xor(xmax, o));
    }
    if ((threadIdx.x & 63) == 0 && xmax > -0x7fffffff) {
        atomicMin(out4 + 0, xmin);
        atomicMin(out4 + 1, y);
        atomicMax(out4 + 2, xmax);
        atomicMax(out4 + 3, y + 1);
    }
}

__global__ void prep_resize_kernel(Src s, int dh, int dw, unsigned char* __restrict__ dst) {
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    if (dx >= dw) return;
    for (int k = 0; k < s.C; ++k) dst[((size_t)dy * dw + dx) * s.C + k] = (unsigned char)resize_sample(s, s.h, s.w, dh, dw, dy, dx, k);
}

// crop + resize to the network input + /255 + background masking + channel stacking of one output pixel: (5, S, S) fp32.
// The one place this arithmetic lives: prep_compose_kernel (one image) and prep_train_compose_kernel (a batch, mirrored
// per image) both call it.
__device__ __forceinline__ void compose_pixel(const Src& rgb, const Src& pm, const Src& om, int ch, int cw, int S, int dy, int dx,
                                              float* __restrict__ out) {
    const int p = resize_sample(pm, ch, cw, S, S, dy, dx, 0), o = resize_sample(om, ch, cw, S, S, dy, dx, 0);
    const bool keep = p >= 128 || o >= 128;                 // (v / 255.) > 0.5
    const size_t plane = (size_t)S * S, q = (size_t)dy * S + dx;
    for (int k = 0; k < 3; ++k) {
        const int v = resize_sample(rgb, ch, cw, S, S, dy, dx, k);
        out[k * plane + q] = keep ? (float)((double)v / 255.0) : 0.f;
    }
    out[3 * plane + q] = (float)((double)p / 255.0);
    out[4 * plane + q] = (float)((double)o / 255.0);
}

__global__ void prep_compose_kernel(Src rgb, Src pm, Src om, int ch, int cw, int S, float* __restrict__ out) {
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    if (dx >= S) return;
    compose_pixel(rgb, pm, om, ch, cw, S, dy, dx, out);
}

// the geometry of BaseDataset.crop (base_data.py:139-160) for corners tl / br on an (H, W) image; cs = side of the crop
struct CropGeom {
    int x1, y1, nx, ny, p1, p2, cw, ch, flip;
};
constexpr int TRAIN_CHUNK = 16;                 // images per launch: their geometry travels as a kernel argument
struct TrainGeom {
    CropGeom g[TRAIN_CHUNK];
};
// the batched prep_compose_kernel: grid (ceil(S / 256), S, images of the chunk)
__global__ void prep_train_compose_kernel(const unsigned char* __restrict__ rgb, const unsigned char* __restrict__ pm,
                                          const unsigned char* __restrict__ om, int H, int W, TrainGeom tg, int S,
                                          float* __restrict__ out) {
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y, b = blockIdx.z;
    if (dx >= S) return;
    const CropGeom g = tg.g[b];
    const size_t px = (size_t)b * H * W;
    const Src r{rgb + px * 3, H, W, 3, g.x1, g.y1, g.nx, g.ny, g.p1, g.p2, g.flip},
              p{pm + px, H, W, 1, g.x1, g.y1, g.nx, g.ny, g.p1, g.p2, g.flip},
              o{om + px, H, W, 1, g.x1, g.y1, g.nx, g.ny, g.p1, g.p2, g.flip};
    compose_pixel(r, p, o, g.ch, g.cw, S, dy, dx, out + (size_t)b * 5 * S * S);
}

// ---- PIL.ImageFilter.GaussianBlur on uint8 images --------------------------------------------------------------------
// (BaseDataset.blur_image, data/base_data.py:122-129.)  PIL approximates the Gaussian by three box blurs along the rows and
// three along the columns, each rounded to uint8, in 24-bit fixed point: with R the integer part of the effective box
// radius, ww the weight of a whole pixel and fw that of the two fractional end pixels (the host computes them, see
// TrainImagePrep.box_params),
//     out[x] = (ww * sum_{|k| <= R} p[x + k] + fw * (p[x - R - 1] + p[x + R + 1]) + 2^23) >> 24,
// indices outside the line taking the nearest end pixel.  The weights add to at most 2^24, so everything fits uint32.
// A workgroup keeps whole lines in LDS (two buffers, the three passes ping-pong between them), so the replicated ends are the
// line's own ends in every pass and R may exceed the line; each thread slides its window over a run of `run` pixels of one
// line.  LDS address of pixel i of line q of block k: k * blk + i * pitch + q.
constexpr int BLUR_MAX_R = 64;
constexpr int BLUR_THREADS = 256;
constexpr int BLUR_LDS_TARGET = 48 * 1024;      // both buffers of a workgroup, when the line allows it: 3 workgroups per CU

__device__ __forceinline__ void box_pass(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int n, int pitch,
                                         int Q, int nblk, int blk, int run, int R, unsigned ww, unsigned fw) {
    const int nruns = (n + run - 1) / run, items = nblk * nruns * Q;
    for (int it = threadIdx.x; it < items; it += BLUR_THREADS) {
        const int q = it % Q, j = (it / Q) % nruns, k = it / (Q * nruns);
        const unsigned char* p = src + k * blk + q;
        unsigned char* o = dst + k * blk + q;
        const int x0 = j * run, x1 = min(n, x0 + run);
        unsigned sum = 0;
        for (int i = x0 - R; i <= x0 + R; ++i) sum += p[clampi(i, 0, n - 1) * pitch];
        for (int x = x0; x < x1; ++x) {
            const unsigned lo = p[clampi(x - R - 1, 0, n - 1) * pitch], hi = p[clampi(x + R + 1, 0, n - 1) * pitch];
            o[x * pitch] = (unsigned char)((ww * sum + fw * (lo + hi) + (1u << 23)) >> 24);
            sum += hi - p[clampi(x - R, 0, n - 1) * pitch];
        }
    }
}
// the three passes; the result is in `b`
__device__ __forceinline__ void box_passes(unsigned char* a, unsigned char* b, int n, int pitch, int Q, int nblk, int blk, int run,
                                           int R, unsigned ww, unsigned fw) {
    box_pass(a, b, n, pitch, Q, nblk, blk, run, R, ww, fw);
    __syncthreads();
    box_pass(b, a, n, pitch, Q, nblk, blk, run, R, ww, fw);
    __syncthreads();
    box_pass(a, b, n, pitch, Q, nblk, blk, run, R, ww, fw);
    __syncthreads();
}

// `rows` lines of `width` bytes between global memory (line stride gstride) and LDS (line stride lstride), in units of V bytes;
// the caller has checked that every address is a multiple of V
template <typename V, bool TO_LDS>
__device__ __forceinline__ void blur_copy(unsigned char* lds, int lstride, unsigned char* g, size_t gstride, int rows, int width) {
    const int per = width / (int)sizeof(V), total = rows * per;
    for (int i = threadIdx.x; i < total; i += BLUR_THREADS) {
        const int r = i / per, c = (i - r * per) * (int)sizeof(V);
        V* l = reinterpret_cast<V*>(lds + r * lstride + c);
        V* m = reinterpret_cast<V*>(g + (size_t)r * gstride + c);
        if (TO_LDS) *l = *m; else *m = *l;
    }
}
template <bool TO_LDS>
__device__ __forceinline__ void blur_move(int vec, unsigned char* lds, int lstride, unsigned char* g, size_t gstride, int rows, int width) {
    if (vec == 16) blur_copy<uint4, TO_LDS>(lds, lstride, g, gstride, rows, width);
    else if (vec == 4) blur_copy<unsigned int, TO_LDS>(lds, lstride, g, gstride, rows, width);
    else blur_copy<unsigned char, TO_LDS>(lds, lstride, g, gstride, rows, width);
}

// rows: a workgroup blurs RB consecutive rows of image blockIdx.y along x.  line = W * C bytes, lpitch = line rounded up to 16.
__global__ __launch_bounds__(BLUR_THREADS) void prep_blur_rows_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                      const int* __restrict__ prm, int H, int W, int C, int RB, int vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char blur_lds[];
    const int b = blockIdx.y, row0 = blockIdx.x * RB, nr = min(RB, H - row0);
    const int line = W * C, lpitch = (line + 15) & ~15;
    const int R = prm[3 * b];
    const unsigned ww = (unsigned)prm[3 * b + 1], fw = (unsigned)prm[3 * b + 2];
    const size_t off = ((size_t)b * H + row0) * line;
    unsigned char* g_in = const_cast<unsigned char*>(src) + off;
    unsigned char *a = blur_lds, *bb = blur_lds + (size_t)RB * lpitch;
    blur_move<true>(vec, a, lpitch, g_in, line, nr, line);
    __syncthreads();
    if (ww != 0) box_passes(a, bb, W, C, C, nr, lpitch, 16, R, ww, fw);       // ww == 0: copy
    blur_move<false>(vec, ww != 0 ? bb : a, lpitch, dst + off, line, nr, line);
}
// columns: a workgroup blurs the strip of SW byte-columns starting at blockIdx.x * SW of image blockIdx.y along y; the strip is
// staged row by row, so global loads and stores stay row-contiguous.  A run of 17 keeps neighbouring runs of a 16-byte strip
// on different LDS banks.
__global__ __launch_bounds__(BLUR_THREADS) void prep_blur_cols_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                      const int* __restrict__ prm, int H, int W, int C, int SW, int vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char blur_lds[];
    const int b = blockIdx.y, c0 = blockIdx.x * SW, line = W * C, sw = min(SW, line - c0);
    const int R = prm[3 * b];
    const unsigned ww = (unsigned)prm[3 * b + 1], fw = (unsigned)prm[3 * b + 2];
    const size_t off = (size_t)b * H * line + c0;
    unsigned char* g_in = const_cast<unsigned char*>(src) + off;
    unsigned char *a = blur_lds, *bb = blur_lds + (size_t)H * SW;
    blur_move<true>(vec, a, SW, g_in, line, H, sw);
    __syncthreads();
    if (ww != 0) box_passes(a, bb, H, SW, sw, 1, 0, 17, R, ww, fw);
    blur_move<false>(vec, ww != 0 ? bb : a, SW, dst + off, line, H, sw);
}

// ---- use_mean_center=True ------------------------------------------------------------------------------------------
// pad_image pastes the uint8 image into a zero float64 canvas so that the crop centre lands on the mean crop centre, the
// crop is then taken from the canvas, and cv2.resize runs its generic float path (float weights, double products, the
// horizontal pass first).  Nothing is materialised here: a canvas pixel is a translated, clipped source pixel.
struct Canvas {                 // canvas rectangle [cx1, cx2) x [cy1, cy2) <- source starting at (sx1, sy1); zero elsewhere
    int ch, cw, cx1, cy1, cx2, cy2, sx1, sy1;
};
struct SrcM {
    const unsigned char* p;
    int h, w, C;
    Canvas cv;
    int x1, y1, nx, ny, p1, p2;        // the crop of the CANVAS (base_data.py:131-162)
    __device__ __forceinline__ double at(int y, int x, int k) const {
        const int cx = x - p1, cy = y - p2;
        if (cx < 0 || cx >= nx || cy < 0 || cy >= ny) return 0.0;
        const int X = x1 + cx, Y = y1 + cy;                           // canvas pixel
        if (X < cv.cx1 || X >= cv.cx2 || Y < cv.cy1 || Y >= cv.cy2) return 0.0;
        return (double)p[((size_t)(cv.sy1 + Y - cv.cy1) * w + (cv.sx1 + X - cv.cx1)) * C + k];
    }
};
__device__ __forceinline__ void lin_coef_f(int d, int n_src, int n_dst, bool clamp_weights, int& s, float& f) {
    const double scale = (double)n_src / (double)n_dst;
    f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f = f - (float)s;
    if (clamp_weights) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    }
}
__device__ __forceinline__ double resize_sample_f64(const SrcM& s, int ch, int cw, int dh, int dw, int dy, int dx, int k) {
    if (cw == dw && ch == dh) return s.at(dy, dx, k);
    if (cw == 2 * dw && ch == 2 * dh)
        return __dmul_rn(__dadd_rn(__dadd_rn(__dadd_rn(s.at(2 * dy, 2 * dx, k), s.at(2 * dy, 2 * dx + 1, k)), s.at(2 * dy + 1, 2 * dx, k)),
                                   s.at(2 * dy + 1, 2 * dx + 1, k)), 0.25);
    int sx, sy;
    float fx, fy;
    lin_coef_f(dx, cw, dw, true, sx, fx);
    lin_coef_f(dy, ch, dh, false, sy, fy);
    const double a0 = (double)(1.0f - fx), a1 = (double)fx, b0 = (double)(1.0f - fy), b1 = (double)fy;
    const int sx1 = min(sx + 1, cw - 1);
    const int y0 = clampi(sy, 0, ch - 1), y1 = clampi(sy + 1, 0, ch - 1);
    const double r0 = __dadd_rn(__dmul_rn(s.at(y0, sx, k), a0), __dmul_rn(s.at(y0, sx1, k), a1));
    const double r1 = __dadd_rn(__dmul_rn(s.at(y1, sx, k), a0), __dmul_rn(s.at(y1, sx1, k), a1));
    return __dadd_rn(__dmul_rn(r0, b0), __dmul_rn(r1, b1));
}
__global__ void prep_compose_mean_kernel(SrcM rgb, SrcM pm, SrcM om, int ch, int cw, int S, float* __restrict__ out) {
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    if (dx >= S) return;
    const double p = resize_sample_f64(pm, ch, cw, S, S, dy, dx, 0) / 255.0, o = resize_sample_f64(om, ch, cw, S, S, dy, dx, 0) / 255.0;
    const bool keep = p > 0.5 || o > 0.5;
    const size_t plane = (size_t)S * S, q = (size_t)dy * S + dx;
    for (int k = 0; k < 3; ++k) {
        const double v = resize_sample_f64(rgb, ch, cw, S, S, dy, dx, k) / 255.0;
        out[k * plane + q] = keep ? (float)v : 0.f;
    }
    out[3 * plane + q] = (float)p;
    out[4 * plane + q] = (float)o;
}

Src plain(const unsigned char* p, int h, int w, int C) { return Src{p, h, w, C, 0, 0, w, h, 0, 0, 0}; }

// geometry of BaseDataset.crop (base_data.py:139-160)
CropGeom crop_geom(int H, int W, int tl_x, int tl_y, int br_x, int br_y, int flip) {
    const int x1 = tl_x > 0 ? tl_x : 0, y1 = tl_y > 0 ? tl_y : 0;
    const int x2 = br_x < W - 1 ? br_x : W - 1, y2 = br_y < H - 1 ? br_y : H - 1;
    const int p1 = tl_x < 0 ? -tl_x : 0, p2 = tl_y < 0 ? -tl_y : 0;
    const int p3 = br_x - W + 1 > 0 ? br_x - W + 1 : 0, p4 = br_y - H + 1 > 0 ? br_y - H + 1 : 0;
    const int nx = x2 > x1 ? x2 - x1 : 0, ny = y2 > y1 ? y2 - y1 : 0;
    return CropGeom{x1, y1, nx, ny, p1, p2, nx + p1 + p3, ny + p2 + p4, flip};
}

bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int chore_prep_masks2bbox(chore_handle* h, const unsigned char* mask0, const unsigned char* mask1, int H, int W, int thres,
                          int* bbox4, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!mask0 || !bbox4 || H <= 0 || W <= 0 || H > 65535) CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_masks2bbox: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int init[4] = {50000, 50000, -100, -100};         // base_data.py:106
    CHORE_HIP_CHECK(h, hipMemcpyAsync(bbox4, init, sizeof(init), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(prep_bbox_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, mask0, mask1, H, W, thres, bbox4);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

int chore_prep_resize_u8(chore_handle* h, const unsigned char* src, int sh, int sw, int C, unsigned char* dst, int dh, int dw,
                         chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!src || !dst || sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || C <= 0 || C > 4 || dh > 65535)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_resize_u8: bad argument");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(prep_resize_kernel, dim3((dw + 255) / 256, dh), dim3(256), 0, s, plain(src, sh, sw, C), dh, dw, dst);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

int chore_prep_crop_compose(chore_handle* h, const unsigned char* rgb, const unsigned char* person_mask,
                            const unsigned char* obj_mask, int H, int W, int tl_x, int tl_y, int br_x, int br_y, int S,
                            float* images, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!rgb || !person_mask || !obj_mask || !images || H <= 0 || W <= 0 || S <= 0 || S > 65535)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_crop_compose: bad argument");
    const CropGeom g = crop_geom(H, W, tl_x, tl_y, br_x, br_y, 0);
    if (g.cw != g.ch || g.cw <= 0)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_crop_compose: the crop is %d x %d, not square (the reference asserts the same)", g.cw, g.ch);
    Src r{rgb, H, W, 3, g.x1, g.y1, g.nx, g.ny, g.p1, g.p2, 0}, p{person_mask, H, W, 1, g.x1, g.y1, g.nx, g.ny, g.p1, g.p2, 0},
        o{obj_mask, H, W, 1, g.x1, g.y1, g.nx, g.ny, g.p1, g.p2, 0};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(prep_compose_kernel, dim3((S + 255) / 256, S), dim3(256), 0, s, r, p, o, g.ch, g.cw, S, images);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

int chore_prep_train_compose(chore_handle* h, const unsigned char* rgb, const unsigned char* person_mask,
                             const unsigned char* obj_mask, int B, int H, int W, const int* tlbr_host, const int* flip_host,
                             int S, float* images, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!rgb || !person_mask || !obj_mask || !images || !tlbr_host || !flip_host || B <= 0 || H <= 0 || W <= 0 || S <= 0 ||
        S > 65535)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_train_compose: bad argument");
    for (int b = 0; b < B; ++b) {               // every image is checked before anything is launched
        const int* t = tlbr_host + 4 * b;
        const CropGeom g = crop_geom(H, W, t[0], t[1], t[2], t[3], 0);
        if (g.cw != g.ch || g.cw <= 0)
            CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_train_compose: the crop of image %d is %d x %d, not square", b, g.cw, g.ch);
    }
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += TRAIN_CHUNK) {
        const int nb = B - b0 < TRAIN_CHUNK ? B - b0 : TRAIN_CHUNK;
        TrainGeom tg = {};
        for (int i = 0; i < nb; ++i) {
            const int* t = tlbr_host + 4 * (b0 + i);
            tg.g[i] = crop_geom(H, W, t[0], t[1], t[2], t[3], flip_host[b0 + i] != 0);
        }
        const size_t px = (size_t)b0 * H * W;
        hipLaunchKernelGGL(prep_train_compose_kernel, dim3((S + 255) / 256, S, nb), dim3(256), 0, s, rgb + px * 3, person_mask + px,
                           obj_mask + px, H, W, tg, S, images + (size_t)b0 * 5 * S * S);
        CHORE_LAUNCH_CHECK(h, s);
    }
    return CHORE_OK;
}

int chore_prep_blur_max_radius(void) { return BLUR_MAX_R; }

size_t chore_prep_blur_workspace_bytes(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 4) return 0;
    return (size_t)B * H * W * C;
}

int chore_prep_blur_u8(chore_handle* h, const unsigned char* src, int B, int H, int W, int C, const int* params, int max_r,
                       unsigned char* dst, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!src || !dst || !params || !workspace || B <= 0 || B > 65535 || H <= 0 || W <= 0 || C <= 0 || C > 4 || max_r < 0)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_blur_u8: bad argument");
    if (max_r > BLUR_MAX_R)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_blur_u8: box radius %d is above the supported %d", max_r, BLUR_MAX_R);
    if ((size_t)H * W * C > 0x7fffffffu) CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_blur_u8: image of %d x %d x %d is too large", H, W, C);
    const int line = W * C, lpitch = (line + 15) & ~15;
    const size_t cu_lds = (size_t)chore_lds_per_cu(h);
    // rows per workgroup / strip width: what fits BLUR_LDS_TARGET; a line too long for that gets a workgroup to itself with up to
    // the CU's LDS, and one too long for that is refused
    int RB = (int)(BLUR_LDS_TARGET / 2 / lpitch);
    RB = RB < 1 ? 1 : (RB > 8 ? 8 : RB);
    if (RB > H) RB = H;
    const size_t lds_rows = 2 * (size_t)RB * lpitch;
    int SW = 64;
    while (SW > 4 && 2 * (size_t)H * SW > (size_t)BLUR_LDS_TARGET) SW >>= 1;
    const size_t lds_cols = 2 * (size_t)H * SW;
    if (lds_rows > cu_lds || lds_cols > cu_lds)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_blur_u8: a line of the %d x %d x %d image does not fit the LDS (%zu / %zu of %zu bytes)",
                   H, W, C, lds_rows, lds_cols, cu_lds);
    unsigned char* ws = (unsigned char*)workspace;
    const bool a16 = aligned_to(src, 16) && aligned_to(dst, 16) && aligned_to(ws, 16) && line % 16 == 0;
    const bool a4 = aligned_to(src, 4) && aligned_to(dst, 4) && aligned_to(ws, 4) && line % 4 == 0;
    const int vec_rows = a16 ? 16 : (a4 ? 4 : 1);
    const int vec_cols = a16 && SW % 16 == 0 ? 16 : (a4 ? 4 : 1);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = CHORE_LAUNCH(h, s, prep_blur_rows_kernel, dim3((H + RB - 1) / RB, B), dim3(BLUR_THREADS), chore_lds(lds_rows, cu_lds),
                              src, ws, params, H, W, C, RB, vec_rows))
        return rc;
    return CHORE_LAUNCH(h, s, prep_blur_cols_kernel, dim3((line + SW - 1) / SW, B), dim3(BLUR_THREADS), chore_lds(lds_cols, cu_lds),
                        (const unsigned char*)ws, dst, params, H, W, C, SW, vec_cols);
}

// use_mean_center=True: the images are first moved so that (cc_x, cc_y) -- the crop centre in the 2048-px space -- lands on
// (mean_x, mean_y) (pad_image, test_data.py:133-160), the crop corners tl / br are those around the mean centre
int chore_prep_crop_compose_mean(chore_handle* h, const unsigned char* rgb, const unsigned char* person_mask,
                                 const unsigned char* obj_mask, int H, int W, double cc_x, double cc_y, double mean_x, double mean_y,
                                 int tl_x, int tl_y, int br_x, int br_y, int S, float* images, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!rgb || !person_mask || !obj_mask || !images || H <= 0 || W <= 0 || S <= 0 || S > 65535)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_crop_compose_mean: bad argument");
    const int kw = 2048, kh = 1536;
    Canvas cv;
    const int tx = (int)(mean_x - cc_x), ty = (int)(mean_y - cc_y);            // astype(int): toward zero
    const int bx = W + tx, by = H + ty;
    cv.cw = bx > kw ? bx : kw; cv.ch = by > kh ? by : kh;
    cv.cx1 = tx > 0 ? tx : 0; cv.cy1 = ty > 0 ? ty : 0;
    cv.cx2 = bx < kw ? bx : kw; cv.cy2 = by < kh ? by : kh;
    cv.sx1 = tx < 0 ? -tx : 0; cv.sy1 = ty < 0 ? -ty : 0;
    const int sx2 = (W - (bx - kw)) < W ? (W - (bx - kw)) : W, sy2 = (H - (by - kh)) < H ? (H - (by - kh)) : H;
    if (cv.cx2 - cv.cx1 != sx2 - cv.sx1 || cv.cy2 - cv.cy1 != sy2 - cv.sy1)    // numpy would refuse the assignment
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_crop_compose_mean: paste rectangles differ (%d x %d vs %d x %d)", cv.cx2 - cv.cx1,
                   cv.cy2 - cv.cy1, sx2 - cv.sx1, sy2 - cv.sy1);
    // geometry of BaseDataset.crop on the canvas
    const int CW = cv.cw, CH = cv.ch;
    const int x1 = tl_x > 0 ? tl_x : 0, y1 = tl_y > 0 ? tl_y : 0;
    const int x2 = br_x < CW - 1 ? br_x : CW - 1, y2 = br_y < CH - 1 ? br_y : CH - 1;
    const int p1 = tl_x < 0 ? -tl_x : 0, p2 = tl_y < 0 ? -tl_y : 0;
    const int p3 = br_x - CW + 1 > 0 ? br_x - CW + 1 : 0, p4 = br_y - CH + 1 > 0 ? br_y - CH + 1 : 0;
    const int nx = x2 > x1 ? x2 - x1 : 0, ny = y2 > y1 ? y2 - y1 : 0;
    const int cw = nx + p1 + p3, ch = ny + p2 + p4;
    if (cw != ch || cw <= 0)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_prep_crop_compose_mean: the crop is %d x %d, not square", cw, ch);
    SrcM r{rgb, H, W, 3, cv, x1, y1, nx, ny, p1, p2}, p{person_mask, H, W, 1, cv, x1, y1, nx, ny, p1, p2},
        o{obj_mask, H, W, 1, cv, x1, y1, nx, ny, p1, p2};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(prep_compose_mean_kernel, dim3((S + 255) / 256, S), dim3(256), 0, s, r, p, o, ch, cw, S, images);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

}  // extern "C"
