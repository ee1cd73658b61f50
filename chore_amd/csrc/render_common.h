// render_common.h -- what the binned triangle rasterisers (render.hip, render_bwd.hip, scene.hip, instances.hip) share: the
// workspace layout, the tile grid, the tile's walk over its bin list that leaves every sample's winning face (or its K nearest)
// in registers, and the texture-and-light shading of a winner with the texel rule the backward differentiates (rb_tex_pos,
// rb_tex_blend).  All files compile these very expressions, so a sample's face, depth and colour are the same bit for bit in
// them.  The setup-and-binning kernel is raster_common.h's, the resolve and id stores raster_store.h's.  render.hip's head
// comment explains the organisation.
#pragma once
#include "raster_common.h"
#include "raster_store.h"

namespace {

constexpr int RB_TW = 16, RB_TH = 16; // output pixels per tile; a wave owns an 8 x 8 quadrant
constexpr int RB_CHUNK = 256;        // list entries looked at per pass
constexpr int RB_TRI_WORDS = 22;     // f[9] + inv[9] + the box: a whole TriSetup

// workspace: TriSetup [B*F] | counters int [B*nb*nb] | lists int [B*nb*nb][F]   (the first two padded to 256 bytes; scene.hip carves on)
struct RenderWs {
    TriSetup* ts;
    int* count;
    int* list;
};
inline RenderWs render_ws(WsCarver& c, int B, int F, int S) {
    const size_t bins = (size_t)B * rb_bins(S) * rb_bins(S);
    return {c.take<TriSetup>((size_t)B * F), c.take<int>(bins), c.raw<int>(bins * F)};
}
// 0 = unsupported shape
inline size_t render_ws_bytes(int B, int F, int size, int ssaa) {
    if (B <= 0 || F <= 0 || size <= 0 || (ssaa != 1 && ssaa != 2) || (long long)size * ssaa > 4096) return 0;
    WsCarver c(nullptr);
    render_ws(c, B, F, size * ssaa);
    return c.bytes;
}
inline bool render_shape_ok(int B, int F, int ts, int size, int ssaa) {
    return !(B <= 0 || B > 65535 || F <= 0 || ts < 2 || size <= 0 || (long long)size * ssaa > 4096 ||
             (long long)B * F > 0x7fffffffLL / 32);
}

// the tile kernels' grid: block x, y = tile of RB_TW x RB_TH output pixels, z = image
inline dim3 rb_tile_grid(int size, int B) { return dim3((size + RB_TW - 1) / RB_TW, (size + RB_TH - 1) / RB_TH, B); }

struct RbShared {                                      // a tile kernel's LDS
    int tri[RB_CHUNK][RB_TRI_WORDS];                   // 22 KB
    int hits[RB_CHUNK];                                // face ids whose box meets this tile
    int wcnt[4];
};

// The staging and the hit tests of a 256-thread workgroup (block x, y = tile, z = image) over its bin's list, shared by the walks
// below.  Every thread must call it; the lane of output pixel (px, py) (rows not flipped; `inside` = it lies in the image) calls
// hit(s, id, zp, w) for every face id of the list that hits its sample s = sy * SS + sx, in the order of the list.
template <int SS, class Hit>
__device__ __forceinline__ void rb_walk_hits(RbShared& sh, const TriSetup* __restrict__ ts, const int* __restrict__ count,
                                             const int* __restrict__ list, int F, int size, float near, float far, int& px,
                                             int& py, bool& inside, Hit&& hit) {
    const int S = size * SS;
    const int b = blockIdx.z;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int lx = (wv & 1) * 8 + (ln & 7), ly = (wv >> 1) * 8 + (ln >> 3);
    px = blockIdx.x * RB_TW + lx; py = blockIdx.y * RB_TH + ly;               // sample-space pixel block (rows not flipped)
    inside = px < size && py < size;
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
        const int nh = raster_compact(meets, fn, sh.hits, sh.wcnt, wv, ln);
        static_assert(sizeof(TriSetup) == RB_TRI_WORDS * sizeof(int), "TriSetup is copied word by word");
        for (int e = threadIdx.x; e < nh * RB_TRI_WORDS; e += 256) {
            const int j = e / RB_TRI_WORDS, k = e - j * RB_TRI_WORDS;
            sh.tri[j][k] = reinterpret_cast<const int*>(tsb + sh.hits[j])[k];
        }
        __syncthreads();
        if (inside) {
            for (int h = 0; h < nh; ++h) {
                // chore_silhouette_fwd at size * ssaa tests a sample against a triangle iff the box meets the sample's aligned
                // 16 x 16 tile.  The same rule here (for ssaa = 2 that tile is the wave's quadrant, so the skip is
                // wave-uniform) keeps even the exact-zero ties of zero-area triangles identical: a sample on the extension of
                // a collinear triangle, outside its box, passes the edge test with all products 0.
                if (sh.tri[h][18] > qx1 || sh.tri[h][19] < qx0 || sh.tri[h][20] > qy1 || sh.tri[h][21] < qy0) continue;
                const float* f = reinterpret_cast<const float*>(sh.tri[h]);
                const float* m = f + 9;
                const int id = sh.hits[h];
#pragma unroll
                for (int sy = 0; sy < SS; ++sy)
#pragma unroll
                    for (int sx = 0; sx < SS; ++sx) {
                        const int s = sy * SS + sx;
                        float w[3], zp;
                        if (!raster_hit(f, m, xp[sx], yp[sy], xf[sx], yf[sy], near, far, w, zp)) continue;
                        hit(s, id, zp, w);
                    }
            }
        }
        __syncthreads();
    }
}

// The walk that leaves every sample's winning face in registers: afterwards the lane holds for each of its SS x SS samples
// s = sy * SS + sx the winning face best[s] (-1 = none), its depth zb[s] (far_z without a face) and its weights wb[s].
template <int SS>
__device__ __forceinline__ void rb_walk(RbShared& sh, const TriSetup* __restrict__ ts, const int* __restrict__ count,
                                        const int* __restrict__ list, int F, int size, float near, float far, int& px, int& py,
                                        bool& inside, float (&zb)[SS * SS], float (&wb)[SS * SS][3], int (&best)[SS * SS]) {
#pragma unroll
    for (int s = 0; s < SS * SS; ++s) {
        zb[s] = far; best[s] = -1;
        wb[s][0] = wb[s][1] = wb[s][2] = 0.f;
    }
    rb_walk_hits<SS>(sh, ts, count, list, F, size, near, far, px, py, inside, [&](int s, int id, float zp, const float* w) {
        // smallest depth, then smallest index: what an in-order z-buffer with `zp < depth` keeps
        if (zp < zb[s] || (zp == zb[s] && best[s] >= 0 && id < best[s])) {
            zb[s] = zp; best[s] = id;
            wb[s][0] = w[0]; wb[s][1] = w[1]; wb[s][2] = w[2];
        }
    });
}

// A candidate (zc, fc) of group gc for one sample's list of the K nearest faces, one per group, in (zp, f) order; an empty
// entry is (inf, -1).  The indices are compile-time constants throughout (a compare-and-shift), so the list stays in registers.
template <int K>
__device__ __forceinline__ void rb_layers_insert(float (&z)[K], int (&f)[K], int (&g)[K], float zc, int fc, int gc) {
    // the group's listed face: a nearer candidate takes it out (and is inserted below), any other candidate is dropped
    bool drop = false, shift = false;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        if (f[i] >= 0 && g[i] == gc) {
            if (zc < z[i] || (zc == z[i] && fc < f[i])) shift = true;
            else drop = true;
        }
        if (shift) {
            z[i] = i + 1 < K ? z[i + 1] : INFINITY;
            f[i] = i + 1 < K ? f[i + 1] : -1;
            g[i] = i + 1 < K ? g[i + 1] : 0;
        }
    }
    if (drop) return;
    // from the back: every entry behind the candidate moves up one place, entry K + 1 falls off.  A NaN depth compares false
    // with every entry, the empty ones included, and is never listed (it never wins in rb_walk either)
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        if (zc < z[i] || (zc == z[i] && fc < f[i])) {
            if (i + 1 < K) { z[i + 1] = z[i]; f[i + 1] = f[i]; g[i + 1] = g[i]; }
            z[i] = zc; f[i] = fc; g[i] = gc;
        }
    }
}

// The walk that leaves every sample's K nearest faces, one per group, in registers (the rule: chore_scene_layers_fwd in
// include/chore_hip.h): lf[s][i] (-1 = none) and their depths lz[s][i] (inf), ascending by (depth, face).  group: this image's
// (F) group ids, or NULL = every face its own group.  The weights are not kept: raster_weights rebuilds them bit for bit.
template <int SS, int K>
__device__ __forceinline__ void rb_walk_layers(RbShared& sh, const TriSetup* __restrict__ ts, const int* __restrict__ count,
                                               const int* __restrict__ list, const int* __restrict__ group, int F, int size,
                                               float near, float far, int& px, int& py, bool& inside, float (&lz)[SS * SS][K],
                                               int (&lf)[SS * SS][K]) {
    int lg[SS * SS][K];
#pragma unroll
    for (int s = 0; s < SS * SS; ++s)
#pragma unroll
        for (int i = 0; i < K; ++i) {
            lz[s][i] = INFINITY; lf[s][i] = -1; lg[s][i] = 0;
        }
    rb_walk_hits<SS>(sh, ts, count, list, F, size, near, far, px, py, inside, [&](int s, int id, float zp, const float*) {
        rb_layers_insert<K>(lz[s], lf[s], lg[s], zp, id, group ? group[id] : id);
    });
}

// The texel rule, once for the forward and the backward (the renderer's gradient is right only while both sample alike).
// Where weights w3 at depth z sample the texture cube of the triangle with vertices f (x y z x y z x y z): the lower tap ti[k] and
// the fraction fr[k] towards the upper one along each axis; tmax = (tsz - 1) - tex_eps.
__device__ __forceinline__ void rb_tex_pos(const float* f, const float* w3, float z, int tsz, float tmax, int* ti, float* fr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float tif = (w3[k] * (float)(tsz - 1)) * (z / f[3 * k + 2]);
        tif = fminf(fmaxf(tif, 0.f), tmax);
        ti[k] = (int)tif;
        fr[k] = tif - (float)ti[k];
    }
}

// the trilinear blend of the eight taps around (ti, fr) of one face's cube `tex` -> c[3]
__device__ __forceinline__ void rb_tex_blend(const float* __restrict__ tex, int tsz, const int* ti, const float* fr, float* c) {
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
}

// colour of face `face` of image b at weights w and depth z: the trilinear blend of its texture cube, times its light
__device__ __forceinline__ void rb_shade(const TriSetup* __restrict__ tsb, const float* __restrict__ textures,
                                         const float* __restrict__ light, int b, int F, int face, int tsz, float tex_eps,
                                         const float* w3, float z, float* c) {
    float fr[3];
    int ti[3];
    rb_tex_pos(tsb[face].f, w3, z, tsz, (float)(tsz - 1) - tex_eps, ti, fr);
    rb_tex_blend(textures + ((size_t)b * F + face) * tsz * tsz * tsz * 3, tsz, ti, fr, c);
    if (light) {
        const float* l = light + ((size_t)b * F + face) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] *= l[k];
    }
}

}  // namespace
