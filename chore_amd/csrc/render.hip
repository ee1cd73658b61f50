// render.hip -- colour / depth / coverage rasterisation of the fitted meshes (forward only, for visualisation).
//
// Replaces what Renderer.render (external/neural_renderer/neural_renderer/renderer.py:237-283) gets from rasterize_rgbad
// (rasterize.py:267-348): the CUDA kernels forward_face_index_map, forward_texture_sampling, forward_background and
// forward_alpha_map (cuda/rasterize_cuda_kernel.cu:24-288) at image size `size * ssaa`, then the vertical flip and the
// 2x2 average of the super-sampled image.  The per-sample hit rule is the one of silhouette.hip (raster_common.h), so the
// winning face of every sample is bit-identical to chore_silhouette_fwd at size * ssaa; organised for this part:
//   * silhouette.hip streams ALL triangles of the image through every 16x16 tile, which is right for the fit (256^2 pixels,
//     <= 5 000 triangles) and hopeless for the demo view (4096^2 samples, ~30 000 triangles).  Here the setup kernel also
//     appends every front-facing, in-view triangle to the lists of the coarse bins (BIN x BIN samples) its box meets.  A list
//     has room for all F triangles, so nothing is ever dropped (the reference keeps 512 per 4x4 block and loses the rest) and
//     the workspace size follows from the shapes alone.  The lists are appended atomically, i.e. in no fixed order; the
//     z-buffer rule is lexicographic (smallest depth, then smallest face index), so the result does not depend on that order.
//   * a workgroup owns 16x16 OUTPUT pixels, a wave one 8x8 quadrant of them, a lane one pixel = its ssaa x ssaa samples.
//     It streams only its bin's list in chunks of 256 ids, keeps the ids whose box meets the tile (ballot + prefix over the
//     four waves), loads those triangles' setup into LDS, and every lane tests the ones whose box meets the aligned 16 x 16
//     samples around its own -- exactly the set chore_silhouette_fwd tests there, and for ssaa = 2 the wave's quadrant, so a
//     wave skips a triangle as a whole, which is why its pixels form a compact square (the divisions of the hit rule run
//     for the whole wave as soon as one lane is inside).  The winner's weights, depth and index
//     stay in registers; texels and light are fetched once per sample after the loop.
//   * resolve in the same launch: the lane averages its samples (rgb, depth, alpha alike, like F.avg_pool2d), flips the
//     row, and stores channel-first.  The super-sampled buffers never reach memory unless sample_face_index is asked for.
#include "raster_common.h"

namespace {

constexpr int RB_BIN = 256;          // coarse bin edge in samples: at most 16 x 16 bins (size * ssaa <= 4096)
constexpr int RB_TW = 16, RB_TH = 16; // output pixels per tile; a wave owns an 8 x 8 quadrant
constexpr int RB_CHUNK = 256;        // list entries looked at per pass
constexpr int RB_TRI_WORDS = 22;     // f[9] + inv[9] + the box: a whole TriSetup

__host__ __device__ inline int rb_bins(int S) { return (S + RB_BIN - 1) / RB_BIN; }

// workspace: TriSetup [B*F] | counters int [B*nb*nb] | lists int [B*nb*nb][F]   (each part padded to 256 bytes)
struct RenderWs {
    TriSetup* ts;
    int* count;
    int* list;
};
__host__ __device__ inline size_t rb_align(size_t x) { return (x + 255) & ~(size_t)255; }
inline RenderWs render_ws(void* workspace, int B, int F, int S) {
    const int nb = rb_bins(S);
    char* p = (char*)workspace;
    RenderWs w;
    w.ts = (TriSetup*)p;
    p += rb_align((size_t)B * F * sizeof(TriSetup));
    w.count = (int*)p;
    p += rb_align((size_t)B * nb * nb * sizeof(int));
    w.list = (int*)p;
    return w;
}

__global__ __launch_bounds__(256) void render_setup_kernel(const float* __restrict__ faces, int B, int F, int S,
                                                           TriSetup* __restrict__ ts, int* __restrict__ count,
                                                           int* __restrict__ list) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * F) return;
    TriSetup t;
#pragma unroll
    for (int k = 0; k < 9; ++k) t.f[k] = faces[(size_t)i * 9 + k];
    tri_setup(t, S);
    ts[i] = t;
    // culled triangles have x0 > x1; a triangle outside the view ends up with an empty clamped box as well
    if (t.x0 > t.x1 || t.y0 > t.y1) return;
    const int b = i / F, fn = i - b * F;
    const int nb = rb_bins(S);
    // 0 <= x0 <= x1 <= S - 1 here, so every bin index is inside [0, nb)
    for (int by = t.y0 / RB_BIN; by <= t.y1 / RB_BIN; ++by)
        for (int bx = t.x0 / RB_BIN; bx <= t.x1 / RB_BIN; ++bx) {
            const size_t bin = ((size_t)b * nb + by) * nb + bx;
            const int slot = atomicAdd(&count[bin], 1);     // < F: a triangle enters a bin's list at most once
            list[bin * F + slot] = fn;
        }
}

template <int SS>
__global__ __launch_bounds__(256) void render_tile_kernel(const TriSetup* __restrict__ ts, const int* __restrict__ count,
                                                          const int* __restrict__ list, const float* __restrict__ textures,
                                                          const float* __restrict__ light, int F, int tsz, int size,
                                                          float near, float far, float tex_eps, float bg0, float bg1,
                                                          float bg2, float* __restrict__ rgb, float* __restrict__ depth_out,
                                                          float* __restrict__ alpha_out, int* __restrict__ sample_face_index) {
    constexpr int NS = SS * SS;
    __shared__ int tri[RB_CHUNK][RB_TRI_WORDS];        // 22 KB
    __shared__ int hits[RB_CHUNK];                     // face ids whose box meets this tile
    __shared__ int wcnt[4];
    const int S = size * SS;
    const int b = blockIdx.z;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int lx = (wv & 1) * 8 + (ln & 7), ly = (wv >> 1) * 8 + (ln >> 3);
    const int px = blockIdx.x * RB_TW + lx, py = blockIdx.y * RB_TH + ly;     // sample-space pixel block (rows not flipped)
    const bool inside = px < size && py < size;
    // the tile in samples; RB_BIN is a multiple of RB_TW * SS and RB_TH * SS, so a tile lies in exactly one bin
    const int sx0 = blockIdx.x * RB_TW * SS, sy0 = blockIdx.y * RB_TH * SS;
    const int sx1 = sx0 + RB_TW * SS - 1, sy1 = sy0 + RB_TH * SS - 1;
    const int nb = rb_bins(S);
    const size_t bin = ((size_t)b * nb + sy0 / RB_BIN) * nb + sx0 / RB_BIN;
    const int cnt = count[bin];
    const int* lst = list + bin * F;
    const TriSetup* tsb = ts + (size_t)b * F;

    float xp[SS], yp[SS], xf[SS], yf[SS];
#pragma unroll
    for (int s = 0; s < SS; ++s) {
        const int xi = px * SS + s, yi = py * SS + s;
        xp[s] = raster_centre(xi, S); yp[s] = raster_centre(yi, S);
        xf[s] = (float)xi; yf[s] = (float)yi;
    }
    float zb[NS], wb[NS][3];
    int best[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        zb[s] = far; best[s] = -1;
        wb[s][0] = wb[s][1] = wb[s][2] = 0.f;
    }

    // the aligned 16 x 16-sample tile (chore_silhouette_fwd's tile at size * ssaa) that holds this lane's samples
    const int qx0 = (px * SS) & ~15, qx1 = qx0 + 15, qy0 = (py * SS) & ~15, qy1 = qy0 + 15;
    for (int c0 = 0; c0 < cnt; c0 += RB_CHUNK) {
        const int n = min(RB_CHUNK, cnt - c0);
        bool meets = false;
        int fn = 0;
        if ((int)threadIdx.x < n) {
            fn = lst[c0 + threadIdx.x];
            const TriSetup* t = tsb + fn;
            const int x0 = t->x0, x1 = t->x1, y0 = t->y0, y1 = t->y1;
            meets = x0 <= sx1 && x1 >= sx0 && y0 <= sy1 && y1 >= sy0;
        }
        const unsigned long long mb = __ballot(meets);
        if (ln == 0) wcnt[wv] = __popcll(mb);
        __syncthreads();
        {
            int base = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) base += q < wv ? wcnt[q] : 0;
            if (meets) hits[base + __popcll(mb & ((1ull << ln) - 1ull))] = fn;
        }
        const int nh = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
        __syncthreads();
        static_assert(sizeof(TriSetup) == RB_TRI_WORDS * sizeof(int), "TriSetup is copied word by word");
        for (int e = threadIdx.x; e < nh * RB_TRI_WORDS; e += 256) {
            const int j = e / RB_TRI_WORDS, k = e - j * RB_TRI_WORDS;
            tri[j][k] = reinterpret_cast<const int*>(tsb + hits[j])[k];
        }
        __syncthreads();
        if (inside) {
            for (int h = 0; h < nh; ++h) {
                // chore_silhouette_fwd at size * ssaa tests a sample against a triangle iff the box meets the sample's aligned
                // 16 x 16 tile.  The same rule here (for ssaa = 2 that tile is the wave's quadrant, so the skip is
                // wave-uniform) keeps even the exact-zero ties of zero-area triangles identical: a sample on the extension of
                // a collinear triangle, outside its box, passes the edge test with all products 0.
                if (tri[h][18] > qx1 || tri[h][19] < qx0 || tri[h][20] > qy1 || tri[h][21] < qy0) continue;
                const float* f = reinterpret_cast<const float*>(tri[h]);
                const float* m = f + 9;
                const int id = hits[h];
#pragma unroll
                for (int sy = 0; sy < SS; ++sy)
#pragma unroll
                    for (int sx = 0; sx < SS; ++sx) {
                        const int s = sy * SS + sx;
                        float w[3], zp;
                        if (!raster_hit(f, m, xp[sx], yp[sy], xf[sx], yf[sy], near, far, w, zp)) continue;
                        // smallest depth, then smallest index: what an in-order z-buffer with `zp < depth` keeps
                        if (zp < zb[s] || (zp == zb[s] && best[s] >= 0 && id < best[s])) {
                            zb[s] = zp; best[s] = id;
                            wb[s][0] = w[0]; wb[s][1] = w[1]; wb[s][2] = w[2];
                        }
                    }
            }
        }
        __syncthreads();
    }
    if (!inside) return;

    float acc[3] = {0.f, 0.f, 0.f}, zacc = 0.f, aacc = 0.f;
    const float tmax = (float)(tsz - 1) - tex_eps;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float c[3] = {bg0, bg1, bg2};
        if (best[s] >= 0) {
            const TriSetup* t = tsb + best[s];
            const float* tex = textures + ((size_t)b * F + best[s]) * tsz * tsz * tsz * 3;
            float fr[3];
            int ti[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float tif = (wb[s][k] * (float)(tsz - 1)) * (zb[s] / t->f[3 * k + 2]);
                tif = fminf(fmaxf(tif, 0.f), tmax);
                ti[k] = (int)tif;
                fr[k] = tif - (float)ti[k];
            }
            c[0] = c[1] = c[2] = 0.f;
#pragma unroll
            for (int pn = 0; pn < 8; ++pn) {
                float w = 1.f;
                int idx[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int up = (pn >> k) & 1;
                    w *= up ? fr[k] : 1.f - fr[k];
                    idx[k] = min(ti[k] + up, tsz - 1);       // the upper neighbour has weight 0 when it would leave the cube
                }
                const float* q = tex + ((idx[0] * tsz + idx[1]) * tsz + idx[2]) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] += w * q[k];
            }
            if (light) {
                const float* l = light + ((size_t)b * F + best[s]) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] *= l[k];
            }
            aacc += 1.f;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += c[k];
        zacc += zb[s];
    }
    constexpr float inv_ns = 1.f / NS;
    const int row = size - 1 - py;                        // rasterize_rgbad flips the rows
    const size_t plane = (size_t)size * size, o = (size_t)row * size + px;
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[((size_t)b * 3 + k) * plane + o] = acc[k] * inv_ns;
    depth_out[(size_t)b * plane + o] = zacc * inv_ns;
    alpha_out[(size_t)b * plane + o] = aacc * inv_ns;
    if (sample_face_index) {
#pragma unroll
        for (int sy = 0; sy < SS; ++sy)
#pragma unroll
            for (int sx = 0; sx < SS; ++sx)
                sample_face_index[((size_t)b * S + (py * SS + sy)) * S + (px * SS + sx)] = best[sy * SS + sx];
    }
}

}  // namespace

extern "C" size_t chore_render_workspace_bytes(int B, int F, int size, int ssaa) {
    if (B <= 0 || F <= 0 || size <= 0 || (ssaa != 1 && ssaa != 2) || (long long)size * ssaa > 4096) return 0;
    const int nb = rb_bins(size * ssaa);
    return rb_align((size_t)B * F * sizeof(TriSetup)) + rb_align((size_t)B * nb * nb * sizeof(int)) +
           (size_t)B * nb * nb * F * sizeof(int);
}

extern "C" int chore_render_fwd(chore_handle* h, const float* tri, const float* textures, const float* light, int B, int F,
                                int ts, int size, int ssaa, float near_z, float far_z, float tex_eps,
                                const float* background3, float* rgb, float* depth, float* alpha, int* sample_face_index,
                                void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!tri || !textures || !background3 || !rgb || !depth || !alpha || !workspace)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_render_fwd: null argument");
    if (ssaa != 1 && ssaa != 2) CHORE_FAIL(h, CHORE_EINVAL, "chore_render_fwd: ssaa must be 1 or 2, got %d", ssaa);
    if (B <= 0 || B > 65535 || F <= 0 || ts < 2 || size <= 0 || (long long)size * ssaa > 4096 ||
        (long long)B * F > 0x7fffffffLL / 32)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_render_fwd: bad sizes B=%d F=%d ts=%d size=%d ssaa=%d", B, F, ts, size, ssaa);
    hipStream_t s = (hipStream_t)stream;
    const int S = size * ssaa, nb = rb_bins(S);
    const RenderWs w = render_ws(workspace, B, F, S);
    CHORE_HIP_CHECK(h, hipMemsetAsync(w.count, 0, (size_t)B * nb * nb * sizeof(int), s));
    const int n = B * F;
    hipLaunchKernelGGL(render_setup_kernel, dim3((n + 255) / 256), dim3(256), 0, s, tri, B, F, S, w.ts, w.count, w.list);
    CHORE_LAUNCH_CHECK(h, s);
    const dim3 grid((size + RB_TW - 1) / RB_TW, (size + RB_TH - 1) / RB_TH, B);
    if (ssaa == 2)
        hipLaunchKernelGGL(render_tile_kernel<2>, grid, dim3(256), 0, s, w.ts, w.count, w.list, textures, light, F, ts, size,
                           near_z, far_z, tex_eps, background3[0], background3[1], background3[2], rgb, depth, alpha,
                           sample_face_index);
    else
        hipLaunchKernelGGL(render_tile_kernel<1>, grid, dim3(256), 0, s, w.ts, w.count, w.list, textures, light, F, ts, size,
                           near_z, far_z, tex_eps, background3[0], background3[1], background3[2], rgb, depth, alpha,
                           sample_face_index);
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
