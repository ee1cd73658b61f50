// render.hip -- colour / depth / coverage rasterisation of the fitted meshes: the forward (the backward is render_bwd.hip).
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
// This file holds the tile kernel's shading loop and the entry point.  The setup kernel is raster_common.h's (raster_setup), the
// walk and the shading live in render_common.h, the resolve and id stores and the ssaa dispatch in raster_store.h; scene.hip,
// instances.hip and render_bwd.hip compile the same helpers.
#include "render_common.h"

namespace {

template <int SS>
__global__ __launch_bounds__(256) void render_tile_kernel(const TriSetup* __restrict__ ts, const int* __restrict__ count,
                                                          const int* __restrict__ list, const float* __restrict__ textures,
                                                          const float* __restrict__ light, int F, int tsz, int size,
                                                          float near, float far, float tex_eps, float bg0, float bg1,
                                                          float bg2, float* __restrict__ rgb, float* __restrict__ depth_out,
                                                          float* __restrict__ alpha_out, int* __restrict__ sample_face_index) {
    constexpr int NS = SS * SS;
    __shared__ RbShared sh;
    const int b = blockIdx.z;
    const TriSetup* tsb = ts + (size_t)b * F;
    int px, py;
    bool inside;
    float zb[NS], wb[NS][3];
    int best[NS];
    rb_walk<SS>(sh, ts, count, list, F, size, near, far, px, py, inside, zb, wb, best);
    if (!inside) return;

    float acc[3] = {0.f, 0.f, 0.f}, zacc = 0.f, aacc = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float c[3] = {bg0, bg1, bg2};
        if (best[s] >= 0) {
            rb_shade(tsb, textures, light, b, F, best[s], tsz, tex_eps, wb[s], zb[s], c);
            aacc += 1.f;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += c[k];
        zacc += zb[s];
    }
    raster_store_resolved<NS>(b, px, py, size, acc, zacc, aacc, rgb, depth_out, alpha_out);
    if (sample_face_index) raster_store_sample_ids<SS>(sample_face_index, b, px, py, size, best);
}

}  // namespace

extern "C" size_t chore_render_workspace_bytes(int B, int F, int size, int ssaa) {
    return render_ws_bytes(B, F, size, ssaa);
}

extern "C" int chore_render_fwd(chore_handle* h, const float* tri, const float* textures, const float* light, int B, int F,
                                int ts, int size, int ssaa, float near_z, float far_z, float tex_eps,
                                const float* background3, float* rgb, float* depth, float* alpha, int* sample_face_index,
                                void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!tri || !textures || !background3 || !rgb || !depth || !alpha || !workspace)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_render_fwd: null argument");
    if (ssaa != 1 && ssaa != 2) CHORE_FAIL(h, CHORE_EINVAL, "chore_render_fwd: ssaa must be 1 or 2, got %d", ssaa);
    if (!render_shape_ok(B, F, ts, size, ssaa))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_render_fwd: bad sizes B=%d F=%d ts=%d size=%d ssaa=%d", B, F, ts, size, ssaa);
    hipStream_t s = (hipStream_t)stream;
    const int S = size * ssaa, nb = rb_bins(S);
    WsCarver c(workspace);
    const RenderWs w = render_ws(c, B, F, S);
    CHORE_HIP_CHECK(h, hipMemsetAsync(w.count, 0, (size_t)B * nb * nb * sizeof(int), s));
    raster_setup(s, tri, B, F, S, w.ts, w.count, w.list);
    CHORE_LAUNCH_CHECK(h, s);
    raster_dispatch_ssaa(ssaa, [&](auto ss) {
        hipLaunchKernelGGL(render_tile_kernel<decltype(ss)::value>, rb_tile_grid(size, B), dim3(256), 0, s, w.ts, w.count, w.list,
                           textures, light, F, ts, size, near_z, far_z, tex_eps, background3[0], background3[1], background3[2], rgb,
                           depth, alpha, sample_face_index);
    });
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
