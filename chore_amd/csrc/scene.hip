// scene.hip -- triangles and points in one image: chore_render_fwd's face layer and chore_splat_fwd's point layer, depth-tested
// against each other per SAMPLE and only then resolved.  Forward only, for the fit's debug views.
//
// The two existing rasterisers resolve their own super-sampling, so their outputs cannot be composited: a silhouette pixel
// is a mixture there and its depth test is lost.  Here nothing new decides a winner: the passes are render.hip's setup and
// binning (render_common.h) and splat.hip's point pass into the 64-bit keys (splat_common.h), unchanged, so each layer is
// bit-identical to the kernel it comes from.  scene_tile_kernel is render_tile_kernel's walk with the winner in
// registers; after the walk the lane loads the keys of its own SS x SS samples (at SS = 2 one 16-byte load per sample row),
// shades both layers with the shared expressions, composes by the rule in include/chore_hip.h, resolves and stores.  The
// super-sampled layers never reach memory.
//   * chore_scene_fwd composes two layers, the nearest face and the nearest point: a translucent face shows the nearest point
//     behind it or the background.  chore_scene_layers_fwd keeps up to 8 faces per sample, optionally one per group of faces
//     (a mesh), and composites them front to back over the point layer: scene_layers_tile_kernel, whose lists are
//     rb_walk_layers' registers.  With one layer it launches scene_tile_kernel.
//   * the call is the clear kernel (keys = empty, bin counters = 0; no hipMemsetAsync, whose byte-memset nodes replay
//     unreliably in hipGraphs, see raster_store.h), the setup kernel, the point pass and the tile kernel, all on the caller's
//     stream; nothing is allocated or read back, so it can be captured.
//   * workspace: render.hip's workspace, padded to 256 bytes, then the keys.
// This file holds the two tile kernels, what they alone share (scene_point_layer: key -> the point's colour, depth, alpha and
// id; scene_over: the blend of a face over what is behind it) and the entry points; everything else is the common headers'.
#include "render_common.h"
#include "splat_common.h"

namespace {

// The point layer of sample s of output pixel (px, py) of image b from its key: false = no point.  Otherwise c becomes the
// point's colour (what shows if it is in front, and under the faces if not), z its depth, a = 1 and id = -2 - n.
template <int SS>
__device__ __forceinline__ bool scene_point_layer(unsigned long long key, const float* __restrict__ pts,
                                                  const float* __restrict__ colors, const float* __restrict__ radius,
                                                  float radius_px, int N, int b, int px, int py, int s, float Sf, float ambient,
                                                  float direct, float near, float far, float* c, float& z, float& a, int& id) {
    if (key == SP_EMPTY) return false;
    const unsigned n = (unsigned)key;
    sp_shade(pts, colors, radius, radius_px, SS, Sf, near, far, (size_t)b * N + n, px * SS + (s % SS), py * SS + (s / SS), ambient,
             direct, c, z);
    a = 1.f;
    id = -2 - (int)n;
    return true;
}

// a face of colour m and opacity o in [0, 1] over what is behind it: c = o m + (1 - o) c, and m itself for an opaque face
__device__ __forceinline__ void scene_over(float o, const float* m, float* c) {
    if (o >= 1.f) {
#pragma unroll
        for (int q = 0; q < 3; ++q) c[q] = m[q];
    } else {
        const float u = __fsub_rn(1.f, o);
#pragma unroll
        for (int q = 0; q < 3; ++q) c[q] = __fadd_rn(__fmul_rn(o, m[q]), __fmul_rn(u, c[q]));
    }
}

template <int SS>
__global__ __launch_bounds__(256) void scene_tile_kernel(const TriSetup* __restrict__ ts, const int* __restrict__ count,
                                                         const int* __restrict__ list, const float* __restrict__ textures,
                                                         const float* __restrict__ light, const float* __restrict__ face_opacity,
                                                         int F, int tsz, const unsigned long long* __restrict__ keys,
                                                         const float* __restrict__ pts, const float* __restrict__ colors,
                                                         const float* __restrict__ radius, float radius_px, int N, float bias,
                                                         int size, float ambient, float near, float far, float tex_eps,
                                                         float bg0, float bg1, float bg2, float* __restrict__ rgb,
                                                         float* __restrict__ depth_out, float* __restrict__ alpha_out,
                                                         int* __restrict__ sample_id) {
    constexpr int NS = SS * SS;
    __shared__ RbShared sh;
    const int S = size * SS;
    const int b = blockIdx.z;
    const TriSetup* tsb = ts + (size_t)b * F;
    int px, py;
    bool inside;
    float zb[NS], wb[NS][3];
    int best[NS];
    rb_walk<SS>(sh, ts, count, list, F, size, near, far, px, py, inside, zb, wb, best);
    if (!inside) return;

    unsigned long long k[NS];
    sp_load_keys<SS>(keys + (size_t)b * S * S, S, px, py, k);
    const float Sf = (float)S;
    const float direct = __fsub_rn(1.f, ambient);
    float acc[3] = {0.f, 0.f, 0.f}, zacc = 0.f, aacc = 0.f;
    int id[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float c[3] = {bg0, bg1, bg2}, z = far, a = 0.f;
        id[s] = -1;
        const bool pt = scene_point_layer<SS>(k[s], pts, colors, radius, radius_px, N, b, px, py, s, Sf, ambient, direct, near, far,
                                              c, z, a, id[s]);
        // equality goes to the face
        if (best[s] >= 0 && !(pt && __fsub_rn(z, bias) < zb[s])) {
            float m[3];
            rb_shade(tsb, textures, light, b, F, best[s], tsz, tex_eps, wb[s], zb[s], m);
            float o = 1.f;
            if (face_opacity) o = fminf(fmaxf(face_opacity[(size_t)b * F + best[s]], 0.f), 1.f);     // NaN -> 0
            scene_over(o, m, c);
            z = zb[s];
            a = pt ? 1.f : o;
            id[s] = best[s];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] += c[q];
        zacc += z;
        aacc += a;
    }
    raster_store_resolved<NS>(b, px, py, size, acc, zacc, aacc, rgb, depth_out, alpha_out);      // chore_render_fwd's resolve
    if (sample_id) raster_store_sample_ids<SS>(sample_id, b, px, py, size, id);
}

// scene_tile_kernel with a list of up to `layers` <= K faces per sample, one per group, instead of the one winner
// (chore_scene_layers_fwd's rule).  The lists live in registers from the walk to the blend and never reach memory.  Only the
// v visible layers are shaded, back to front, in a loop that is NOT unrolled: it picks layer i out of the registers by a chain of
// selects over compile-time indices, so the shading code exists once per sample and nothing is indexed dynamically.
template <int SS, int K>
__global__ __launch_bounds__(256) void scene_layers_tile_kernel(
    const TriSetup* __restrict__ ts, const int* __restrict__ count, const int* __restrict__ list, const float* __restrict__ textures,
    const float* __restrict__ light, const float* __restrict__ face_opacity, const int* __restrict__ face_group, int layers, int F,
    int tsz, const unsigned long long* __restrict__ keys, const float* __restrict__ pts, const float* __restrict__ colors,
    const float* __restrict__ radius, float radius_px, int N, float bias, int size, float ambient, float near, float far,
    float tex_eps, float bg0, float bg1, float bg2, float* __restrict__ rgb, float* __restrict__ depth_out,
    float* __restrict__ alpha_out, int* __restrict__ sample_id) {
    constexpr int NS = SS * SS;
    __shared__ RbShared sh;
    const int S = size * SS;
    const int b = blockIdx.z;
    const TriSetup* tsb = ts + (size_t)b * F;
    int px, py;
    bool inside;
    float lz[NS][K];
    int lf[NS][K];
    rb_walk_layers<SS, K>(sh, ts, count, list, face_group ? face_group + (size_t)b * F : nullptr, F, size, near, far, px, py, inside,
                          lz, lf);
    if (!inside) return;

    unsigned long long k[NS];
    sp_load_keys<SS>(keys + (size_t)b * S * S, S, px, py, k);
    const float Sf = (float)S;
    const float direct = __fsub_rn(1.f, ambient);
    const float* opb = face_opacity ? face_opacity + (size_t)b * F : nullptr;
    auto opacity = [&](int f) { return opb ? fminf(fmaxf(opb[f], 0.f), 1.f) : 1.f; };      // NaN -> 0
    float acc[3] = {0.f, 0.f, 0.f}, zacc = 0.f, aacc = 0.f;
    int id[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float c[3] = {bg0, bg1, bg2}, z = far, a = 0.f;
        id[s] = -1;
        const bool pt = scene_point_layer<SS>(k[s], pts, colors, radius, radius_px, N, b, px, py, s, Sf, ambient, direct, near, far,
                                              c, z, a, id[s]);
        // j listed faces lie before the point (equality goes to the face); depths ascend, so they are the first j
        const float zt = __fsub_rn(z, bias);
        int j = 0;
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (q < layers && lf[s][q] >= 0 && !(pt && zt < lz[s][q])) j = q + 1;
        // v of them are visible: up to the first opaque one
        int v = j;
        bool cut = false;
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (q < j && !cut && opacity(lf[s][q]) >= 1.f) {
                v = q + 1;
                cut = true;
            }
        if (v > 0) {
            const int xi = px * SS + (s % SS), yi = py * SS + (s / SS);
            float al = 0.f;
#pragma unroll 1
            for (int i = v - 1; i >= 0; --i) {
                float zi = lz[s][0];
                int fi = lf[s][0];
#pragma unroll
                for (int q = 1; q < K; ++q)
                    if (q == i) {
                        zi = lz[s][q];
                        fi = lf[s][q];
                    }
                const float* tf = reinterpret_cast<const float*>(tsb + fi);
                float w[3], zr, m[3];
                raster_weights(tf, tf + 9, (float)xi, (float)yi, w, zr);       // the walk's own expressions: zr == zi
                rb_shade(tsb, textures, light, b, F, fi, tsz, tex_eps, w, zi, m);
                const float o = opacity(fi);
                scene_over(o, m, c);
                al = __fadd_rn(o, __fmul_rn(__fsub_rn(1.f, o), al));
            }
            z = lz[s][0];
            a = (pt || cut) ? 1.f : al;
            id[s] = lf[s][0];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] += c[q];
        zacc += z;
        aacc += a;
    }
    raster_store_resolved<NS>(b, px, py, size, acc, zacc, aacc, rgb, depth_out, alpha_out);      // chore_render_fwd's resolve
    if (sample_id) raster_store_sample_ids<SS>(sample_id, b, px, py, size, id);
}

// workspace: the render layout, padded to 256 bytes | the splat keys
struct SceneWs { RenderWs r; unsigned long long* keys; size_t bytes; };
SceneWs scene_ws(void* base, int B, int F, int size, int ssaa) {
    WsCarver c(base);
    const RenderWs r = render_ws(c, B, F, size * ssaa);
    c.pad();
    return {r, (unsigned long long*)c.raw<char>(splat_key_bytes(B, size, ssaa)), c.bytes};
}

}  // namespace

extern "C" size_t chore_scene_workspace_bytes(int B, int F, int N, int size, int ssaa) {
    if (render_ws_bytes(B, F, size, ssaa) == 0 || !render_shape_ok(B, F, 2, size, ssaa) || !splat_shape_ok(B, N, size, ssaa)) return 0;
    return scene_ws(nullptr, B, F, size, ssaa).bytes;
}

// both entry points: the checks, the three shared passes and the tile kernel for `layers` (1 = scene_tile_kernel)
static int scene_fwd(chore_handle* h, const char* who, const float* tri, const float* textures, const float* light,
                     const float* face_opacity, int B, int F, int ts, const float* pts, const float* point_rgb, const float* radius,
                     float radius_px, int N, float point_depth_bias, int size, int ssaa, float ambient, float near_z, float far_z,
                     float tex_eps, const float* background3, const int* face_group, int layers, float* rgb, float* depth,
                     float* alpha, int* sample_id, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!tri || !textures || !pts || !background3 || !rgb || !depth || !alpha || !workspace)
        CHORE_FAIL(h, CHORE_EINVAL, "%s: null argument", who);
    if (layers < 1 || layers > 8) CHORE_FAIL(h, CHORE_EINVAL, "%s: face_layers must lie in 1..8, got %d", who, layers);
    if (ssaa != 1 && ssaa != 2) CHORE_FAIL(h, CHORE_EINVAL, "%s: ssaa must be 1 or 2, got %d", who, ssaa);
    if (!render_shape_ok(B, F, ts, size, ssaa) || !splat_shape_ok(B, N, size, ssaa))
        CHORE_FAIL(h, CHORE_EINVAL, "%s: bad sizes B=%d F=%d ts=%d N=%d size=%d ssaa=%d", who, B, F, ts, N, size, ssaa);
    if (int rc = sp_check_args(h, who, ambient, near_z, far_z, radius, radius_px)) return rc;
    if (!(point_depth_bias >= 0.f))
        CHORE_FAIL(h, CHORE_EINVAL, "%s: point_depth_bias must be >= 0, got %g", who, (double)point_depth_bias);
    hipStream_t s = (hipStream_t)stream;
    const int S = size * ssaa, nb = rb_bins(S);
    const SceneWs sw = scene_ws(workspace, B, F, size, ssaa);
    const RenderWs& w = sw.r;
    unsigned long long* keys = sw.keys;
    const size_t nkeys = (size_t)B * S * S, ncount = (size_t)B * nb * nb;
    raster_clear(s, (nkeys + 1) / 2 > ncount ? (nkeys + 1) / 2 : ncount, keys, nkeys, w.count, ncount);
    CHORE_LAUNCH_CHECK(h, s);
    raster_setup(s, tri, B, F, S, w.ts, w.count, w.list);
    CHORE_LAUNCH_CHECK(h, s);
    splat_pass(s, pts, radius, radius_px, B, N, S, ssaa, near_z, far_z, keys);
    CHORE_LAUNCH_CHECK(h, s);
    raster_dispatch_ssaa(ssaa, [&](auto ss) {
        constexpr int SS = decltype(ss)::value;
        const dim3 grid = rb_tile_grid(size, B);
        if (layers == 1) {
            hipLaunchKernelGGL(scene_tile_kernel<SS>, grid, dim3(256), 0, s, w.ts, w.count, w.list, textures, light, face_opacity, F, ts,
                               keys, pts, point_rgb, radius, radius_px, N, point_depth_bias, size, ambient, near_z, far_z, tex_eps,
                               background3[0], background3[1], background3[2], rgb, depth, alpha, sample_id);
        } else {
            // capacities 2, 4 and 8; a request between two of them runs in the larger with its list cut at `layers`
            const auto kernel = layers <= 2 ? scene_layers_tile_kernel<SS, 2>
                              : layers <= 4 ? scene_layers_tile_kernel<SS, 4> : scene_layers_tile_kernel<SS, 8>;
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, w.ts, w.count, w.list, textures, light, face_opacity, face_group, layers,
                               F, ts, keys, pts, point_rgb, radius, radius_px, N, point_depth_bias, size, ambient, near_z, far_z,
                               tex_eps, background3[0], background3[1], background3[2], rgb, depth, alpha, sample_id);
        }
    });
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}

extern "C" int chore_scene_fwd(chore_handle* h, const float* tri, const float* textures, const float* light,
                               const float* face_opacity, int B, int F, int ts, const float* pts, const float* point_rgb,
                               const float* radius, float radius_px, int N, float point_depth_bias, int size, int ssaa,
                               float ambient, float near_z, float far_z, float tex_eps, const float* background3, float* rgb,
                               float* depth, float* alpha, int* sample_id, void* workspace, chore_stream_t stream) {
    return scene_fwd(h, "chore_scene_fwd", tri, textures, light, face_opacity, B, F, ts, pts, point_rgb, radius, radius_px, N,
                     point_depth_bias, size, ssaa, ambient, near_z, far_z, tex_eps, background3, nullptr, 1, rgb, depth, alpha,
                     sample_id, workspace, stream);
}

extern "C" int chore_scene_layers_fwd(chore_handle* h, const float* tri, const float* textures, const float* light,
                                      const float* face_opacity, int B, int F, int ts, const float* pts, const float* point_rgb,
                                      const float* radius, float radius_px, int N, float point_depth_bias, int size, int ssaa,
                                      float ambient, float near_z, float far_z, float tex_eps, const float* background3,
                                      const int* face_group, int face_layers, float* rgb, float* depth, float* alpha,
                                      int* sample_id, void* workspace, chore_stream_t stream) {
    return scene_fwd(h, "chore_scene_layers_fwd", tri, textures, light, face_opacity, B, F, ts, pts, point_rgb, radius, radius_px,
                     N, point_depth_bias, size, ssaa, ambient, near_z, far_z, tex_eps, background3, face_group, face_layers, rgb,
                     depth, alpha, sample_id, workspace, stream);
}
