// render_bwd.hip -- the backward of chore_render_fwd: gradients of rgb / depth / alpha with respect to the projected
// triangles, the texture cubes and the per-face light.
//
// Replaces what RasterizeFunction.backward (external/neural_renderer/neural_renderer/rasterize.py:114-170) gets from the CUDA
// kernels backward_pixel_map (cuda/rasterize_cuda_kernel.cu:290-549, alpha + rgb), backward_textures (:551-586) and
// backward_depth_map (:588-638), on the sample grid S = size * ssaa of the forward, with the forward's flip and average
// pulled back first.  Same mathematics, organised for this part:
//   * the forward keeps no per-sample image, so a first launch re-shades every sample from sample_face_index into the
//     workspace (colour + alpha as one float4) and spreads the upstream gradients of its output pixel over it (rgb + alpha
//     as one float4, depth as a float), divided by ssaa^2, from row size-1-r: the walk then reads 32 bytes per sample.
//   * the pixel-map term is the edge walk of silhouette.hip (raster_common.h: a workgroup per triangle, a wave per
//     (edge, axis) walk, eight samples of a scan line in flight), with diff_grad summed over alpha, r, g, b before its gate.
//     One writer per triangle, as in the reference.
//   * the reference scatters the depth and texture terms per pixel with float atomicAdd, whose order changes from run to
//     run.  Here a workgroup owns a triangle and gathers: it walks the 16 x 16-sample tiles that the triangle's box meets
//     (exactly where the forward tested it), takes the samples whose winner it is, rebuilds their weights and depth with the
//     forward's expressions, and sums per thread in a fixed order, then over the workgroup by a fixed tree.  Texels are
//     accumulated eight at a time in registers (ts = 2: one pass over the box; the box is walked ceil(ts^3 / 8) times).
//     A triangle that owns most of a large image is walked by its one workgroup alone.
#include "render_common.h"

namespace {

// workspace: TriSetup [B*F], padded to 256 bytes | colour + alpha float4 [B*S*S] | d rgb + d alpha float4 [B*S*S] | d depth float [B*S*S]
struct RenderBwdWs { TriSetup* ts; float4* col; float4* grad; float* gdepth; size_t bytes; };
inline RenderBwdWs render_bwd_ws(void* workspace, int B, int F, int S) {
    const size_t n = (size_t)B * S * S;
    WsCarver c(workspace);
    return {c.take<TriSetup>((size_t)B * F), c.raw<float4>(n), c.raw<float4>(n), c.raw<float>(n), c.bytes};
}

// thread = sample (x fastest): its colour and alpha as the forward produced them, and its share of the upstream gradients
__global__ __launch_bounds__(256) void rbw_sample_kernel(const TriSetup* __restrict__ ts, const float* __restrict__ textures,
                                                         const float* __restrict__ light, const int* __restrict__ fim, int F,
                                                         int tsz, int size, int ss, float tex_eps, float bg0, float bg1,
                                                         float bg2, const float* __restrict__ g_rgb,
                                                         const float* __restrict__ g_depth, const float* __restrict__ g_alpha,
                                                         float4* __restrict__ col, float4* __restrict__ grad,
                                                         float* __restrict__ gdepth) {
    const int S = size * ss;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= S || y >= S) return;
    const size_t q = ((size_t)b * S + y) * S + x;
    const int fn = fim[q];
    const bool hit = fn >= 0 && fn < F;
    float c[3] = {bg0, bg1, bg2};
    if (!g_rgb) c[0] = c[1] = c[2] = 0.f;          // no colour term: nothing to shade
    else if (hit) {
        const TriSetup* tsb = ts + (size_t)b * F;
        float w[3], zp;
        raster_weights(tsb[fn].f, tsb[fn].inv, (float)x, (float)y, w, zp);
        rb_shade(tsb, textures, light, b, F, fn, tsz, tex_eps, w, zp, c);
    }
    col[q] = make_float4(c[0], c[1], c[2], hit ? 1.f : 0.f);
    const float inv_ns = 1.f / (float)(ss * ss);
    const size_t plane = (size_t)size * size, o = (size_t)(size - 1 - y / ss) * size + x / ss;
    float g[3] = {0.f, 0.f, 0.f};
    if (g_rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = g_rgb[((size_t)b * 3 + k) * plane + o] * inv_ns;
    }
    grad[q] = make_float4(g[0], g[1], g[2], g_alpha ? g_alpha[(size_t)b * plane + o] * inv_ns : 0.f);
    gdepth[q] = g_depth ? g_depth[(size_t)b * plane + o] * inv_ns : 0.f;
}

// what the shared edge walk sees of the sample image: alpha first, then r, g, b, summed before the gate
struct RenderImg {
    const int* fim; const float4* col; const float4* grad; int size;
    typedef float4 Ref;
    struct Px { float4 c, g; };
    __device__ __forceinline__ size_t at(int axis, int d0, int d1) const {
        return axis == 0 ? (size_t)d1 * size + d0 : (size_t)d0 * size + d1;
    }
    __device__ __forceinline__ int face(size_t q) const { return fim[q]; }
    __device__ __forceinline__ Ref ref(size_t q) const { return col[q]; }
    __device__ __forceinline__ Px load(size_t q) const { return Px{col[q], grad[q]}; }
    __device__ __forceinline__ float diff(const Px& p, const Ref& r) const {
        float d = (p.c.w - r.w) * p.g.w;
        d += (p.c.x - r.x) * p.g.x;
        d += (p.c.y - r.y) * p.g.y;
        d += (p.c.z - r.z) * p.g.z;
        return d;
    }
};

__global__ __launch_bounds__(384) void rbw_pixel_map_kernel(const float* __restrict__ faces, const int* __restrict__ fim,
                                                            const float4* __restrict__ col, const float4* __restrict__ grad,
                                                            int F, int S, float eps, float* __restrict__ grad_tri) {
    const int i = blockIdx.x;
    const int b = i / F, fn = i - b * F;
    __shared__ float part[6][2];
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = faces[(size_t)i * 9 + k];
    const size_t img = (size_t)b * S * S;
    const RenderImg im{fim + img, col + img, grad + img, S};
    raster_pixel_map_bwd(im, f, fn, tri_backside(f), eps, part, grad_tri + (size_t)i * 9);
}

constexpr int RBW_TEXELS = 8;                            // texels accumulated per walk over the box
constexpr int RBW_NACC = 3 + 3 + 3 * RBW_TEXELS;         // depth (per vertex), light, texels x rgb

// One workgroup per triangle: the depth term (-> grad_tri, added to what is there if `accumulate`), grad_textures and
// grad_light (either may be NULL) of the samples it won.  thread = one sample of a 16 x 16 tile.
__global__ __launch_bounds__(256) void rbw_gather_kernel(const TriSetup* __restrict__ ts, const float* __restrict__ textures,
                                                         const float* __restrict__ light, const int* __restrict__ fim,
                                                         const float4* __restrict__ grad, const float* __restrict__ gdepth,
                                                         int F, int tsz, int S, float tex_eps, int do_rgb, int accumulate,
                                                         float* __restrict__ grad_tri, float* __restrict__ grad_textures,
                                                         float* __restrict__ grad_light) {
    __shared__ float red[4][RBW_NACC];
    __shared__ TriSetup tsh;
    const int i = blockIdx.x;
    const int b = i / F, fn = i - b * F;
    const int tid = threadIdx.x;
    if (tid < RB_TRI_WORDS) reinterpret_cast<int*>(&tsh)[tid] = reinterpret_cast<const int*>(ts + i)[tid];
    __syncthreads();
    const TriSetup& t = tsh;
    const int nt3 = tsz * tsz * tsz;
    const bool empty = t.x0 > t.x1 || t.y0 > t.y1;      // culled or out of view: it won no sample
    const int passes = (do_rgb && grad_textures) ? (nt3 + RBW_TEXELS - 1) / RBW_TEXELS : 1;
    const size_t img = (size_t)b * S * S;
    const float tmax = (float)(tsz - 1) - tex_eps;
    float lt[3] = {1.f, 1.f, 1.f};
    if (light) {
#pragma unroll
        for (int k = 0; k < 3; ++k) lt[k] = light[(size_t)i * 3 + k];
    }
    const float* tex = textures + (size_t)i * nt3 * 3;
    // a triangle that won no sample: zeros (its texels are zero already), and nothing to sum
    auto nothing = [&]() {
        if (!accumulate && tid < 9) grad_tri[(size_t)i * 9 + tid] = 0.f;
        if (grad_light && tid < 3) grad_light[(size_t)i * 3 + tid] = 0.f;
    };
    if (empty) { nothing(); return; }

    for (int pass = 0; pass < passes; ++pass) {
        float acc[RBW_NACC];
#pragma unroll
        for (int k = 0; k < RBW_NACC; ++k) acc[k] = 0.f;
        // the forward tested this triangle on every aligned 16 x 16 tile its box meets: raster_for_each_won_pixel walks those
        const int mine = raster_for_each_won_pixel(t, fim + img, fn, S, [&](size_t p, int, int, const float* w, float zp) {
            const size_t q = img + p;
            if (pass == 0) raster_depth_bwd_sample(gdepth[q], w, zp, acc);
            if (!do_rgb) return;
            const float4 g4 = grad[q];
            const float g[3] = {g4.x, g4.y, g4.z};
            float fr[3];
            int ti[3];
            rb_tex_pos(t.f, w, zp, tsz, tmax, ti, fr);      // the forward's sampling position: rb_shade calls the same
            if (pass == 0 && grad_light) {       // d light = d rgb x the blended texel
                float c[3];
                rb_tex_blend(tex, tsz, ti, fr, c);
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[3 + k] += g[k] * c[k];
            }
            if (grad_textures) {
                const float gl[3] = {g[0] * lt[0], g[1] * lt[1], g[2] * lt[2]};
#pragma unroll
                for (int u = 0; u < RBW_TEXELS; ++u) {
                    const int lin = pass * RBW_TEXELS + u;           // texel (i0, i1, i2), uniform
                    const int i0 = lin / (tsz * tsz), i1 = (lin / tsz) % tsz, i2 = lin % tsz;
                    const int id[3] = {i0, i1, i2};
                    float wt = 1.f;
#pragma unroll
                    for (int k = 0; k < 3; ++k)      // the weight of index id[k] along axis k: lower + upper tap
                        wt *= (id[k] == ti[k] ? 1.f - fr[k] : 0.f) + (id[k] == min(ti[k] + 1, tsz - 1) ? fr[k] : 0.f);
#pragma unroll
                    for (int k = 0; k < 3; ++k) acc[6 + 3 * u + k] += wt * gl[k];
                }
            }
        });
        // most triangles of a fine mesh win no sample (hidden, or between the sample centres)
        if (!__syncthreads_or(mine)) { nothing(); return; }
        // the workgroup's sums: a fixed butterfly per wave, then the four waves in order
        raster_wg_sum<RBW_NACC>(acc, red);
        if (pass == 0 && tid == 0) {
            // backward_depth_map, with A_k = sum d depth * w_k * depth^2 in red[0][0..2]
            float g9[9];
            raster_depth_bwd_face(t, red[0], S, g9);
            float* out = grad_tri + (size_t)i * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) out[k] = accumulate ? out[k] + g9[k] : g9[k];
        }
        if (pass == 0 && grad_light && tid < 3) grad_light[(size_t)i * 3 + tid] = red[0][3 + tid];
        if (grad_textures && tid < 3 * RBW_TEXELS && pass * RBW_TEXELS * 3 + tid < nt3 * 3) {
            if (do_rgb) grad_textures[(size_t)i * nt3 * 3 + pass * RBW_TEXELS * 3 + tid] = red[0][6 + tid];
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" size_t chore_render_bwd_workspace_bytes(int B, int F, int ts, int size, int ssaa) {
    if ((ssaa != 1 && ssaa != 2) || !render_shape_ok(B, F, ts, size, ssaa)) return 0;
    return render_bwd_ws(nullptr, B, F, size * ssaa).bytes;
}

extern "C" int chore_render_bwd(chore_handle* h, const float* tri, const float* textures, const float* light,
                                const int* sample_face_index, int B, int F, int ts, int size, int ssaa, float near_z,
                                float far_z, float tex_eps, float eps, const float* background3, const float* grad_rgb,
                                const float* grad_depth, const float* grad_alpha, float* grad_tri, float* grad_textures,
                                float* grad_light, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    (void)near_z; (void)far_z;      // a winner passed the forward's near / far test; kept in the signature beside the forward's
    if (!tri || !textures || !sample_face_index || !background3 || !grad_tri || !workspace)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_render_bwd: null argument");
    if (ssaa != 1 && ssaa != 2) CHORE_FAIL(h, CHORE_EINVAL, "chore_render_bwd: ssaa must be 1 or 2, got %d", ssaa);
    if (!render_shape_ok(B, F, ts, size, ssaa))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_render_bwd: bad sizes B=%d F=%d ts=%d size=%d ssaa=%d", B, F, ts, size, ssaa);
    hipStream_t s = (hipStream_t)stream;
    const int S = size * ssaa, n = B * F;
    const size_t ntex = (size_t)n * ts * ts * ts * 3;
    const bool pixel_map = grad_rgb || grad_alpha, gather = grad_rgb || grad_depth;
    // the gather writes the texels of the triangles that are in view; everything else, and everything without a colour
    // gradient, is zero.  grad_tri is written by whichever launch runs first.
    if (grad_textures) CHORE_HIP_CHECK(h, hipMemsetAsync(grad_textures, 0, ntex * sizeof(float), s));
    if (grad_light && !grad_rgb) CHORE_HIP_CHECK(h, hipMemsetAsync(grad_light, 0, (size_t)n * 3 * sizeof(float), s));
    if (!pixel_map && !gather) {
        CHORE_HIP_CHECK(h, hipMemsetAsync(grad_tri, 0, (size_t)n * 9 * sizeof(float), s));
        return CHORE_OK;
    }
    const RenderBwdWs w = render_bwd_ws(workspace, B, F, S);
    raster_setup(s, tri, B, F, S, w.ts);
    CHORE_LAUNCH_CHECK(h, s);
    hipLaunchKernelGGL(rbw_sample_kernel, dim3((S + 63) / 64, (S + 3) / 4, B), dim3(256), 0, s, w.ts, textures, light,
                       sample_face_index, F, ts, size, ssaa, tex_eps, background3[0], background3[1], background3[2], grad_rgb,
                       grad_depth, grad_alpha, w.col, w.grad, w.gdepth);
    CHORE_LAUNCH_CHECK(h, s);
    if (pixel_map) {
        hipLaunchKernelGGL(rbw_pixel_map_kernel, dim3(n), dim3(384), 0, s, tri, sample_face_index, w.col, w.grad, F, S, eps,
                           grad_tri);
        CHORE_LAUNCH_CHECK(h, s);
    }
    if (gather) {
        hipLaunchKernelGGL(rbw_gather_kernel, dim3(n), dim3(256), 0, s, w.ts, textures, light, sample_face_index, w.grad,
                           w.gdepth, F, ts, S, tex_eps, grad_rgb ? 1 : 0, pixel_map ? 1 : 0, grad_tri, grad_textures,
                           grad_light);
        CHORE_LAUNCH_CHECK(h, s);
    }
    return CHORE_OK;
}
