// mesh_dist.hip -- exact unsigned point-to-triangle-mesh distance on the device, fp32, gfx950.
//
// What the training-data sampler of the reference gets from igl.signed_distance (|S|, I, C) and from
// trimesh.proximity.ProximityQuery.vertex (preprocess/boundary_sampler.py:45-64): for every query point the distance to
// the SURFACE of the mesh, a triangle that attains it, the closest point on that triangle, and the nearest mesh VERTEX.
// Brute force over all triangles -- no tree, no culling: the result is the minimum over every triangle by construction.
//
//   record_kernel   one record of 16 floats (one 64-byte line) per triangle and image: a, ab, ac, guarded reciprocals of
//                   the three squared edge lengths and the three coefficients of the plane's barycentric coordinates.
//                   The scalars are formed in fp64 from the fp32 edges, so a zero-area triangle is recognised exactly.
//   dist_kernel     grid (point tiles, face chunks, B): 256 threads keep MD_P points each in registers, stream their chunk
//                   of records through LDS in tiles of MD_TILE and read them at wave-uniform addresses (broadcast).  Every
//                   candidate is the distance to a POINT OF THE TRIANGLE -- the clamped projections on the three edges and,
//                   where all three barycentric coordinates are positive, the projection on the plane -- so rounding in a
//                   coordinate can move the foot point along the triangle (a second-order change of the distance) but can
//                   never report less than the triangle's distance, and a triangle that degenerates to a segment or a
//                   point needs no special case: its plane coefficients are zero and its edges are what is left.
//                   Result per (chunk, point): a 64-bit key, squared distance bits above the face index, so that the
//                   minimum of keys is "smallest fp32 squared distance, then smallest face index".
//   finish_kernel   minimum over the chunks' keys, sqrt, closest point of the winning triangle (same arithmetic).
//   vertex_kernel   nearest vertex, tiled through LDS, first smallest squared distance (only when vert_idx is asked for).
//
// chore_mesh_sdf_fwd is the same call plus the generalized winding number (Jacobson et al. 2013): the WIND instantiations of the
// three kernels' bodies (record_kernel_w, dist_kernel_w, finish_kernel_w).  In the loop of dist_kernel_w every triangle also adds
// atan2(a.(b x c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|), half its signed solid angle (van Oosterom & Strackee 1983; a, b,
// c = corners minus the point), to a per-point float; every (chunk, point) stores that partial sum beside its key and
// finish_kernel_w adds the chunks in ascending order and divides by 2 pi: no atomics, the bits depend on the shapes and the inputs alone.  a, b, c are formed from the corners themselves (a second
// record per triangle, RecW, beside the first in LDS), one rounding each and the same value in every triangle that shares the
// corner: next to an edge the two large angles of its triangles then err alike and cancel, which a + ab - p would not give.
// A triangle whose fp32 edges ab, ac are exactly parallel (repeated index, zero area; recognised in fp64 by record_kernel,
// RecW::area = 0) has its determinant forced to +-0, a point on a corner has one of a, b, c = 0: the determinant is +-0 and the
// denominator +0, so atan2 gives +-0 without a special case.
// The unsigned instantiations are the kernels as they were (same registers, LDS, occupancy: DESIGN.md, 'Mesh distance').
#include "common.h"

namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_P = 2;                          // points per thread
constexpr int MD_PTS = MD_THREADS * MD_P;        // points per workgroup
constexpr int MD_TILE = 128;                     // records per LDS tile (8 KiB)
constexpr int MD_REC = 16;                       // floats per record
constexpr int MD_VTILE = 1024;                   // vertices per LDS tile of vertex_kernel (12 KiB)
constexpr int MD_WANT_GROUPS = 2048;             // workgroups the split over face chunks aims for (8 per CU on 256 CUs)
constexpr int MD_MAX_CHUNKS = 64;

struct Rec {
    float ax, ay, az, abx, aby, abz, acx, acy, acz;
    float inv_ab, inv_ac, inv_bc;   // 1 / |edge|^2, 0 for an edge of length 0
    float k1, k2, k3;               // v = k1 d1 - k2 d2, w = k3 d2 - k2 d1 with d1 = ab.ap, d2 = ac.ap; all 0 = no interior
    float pad;
};
struct RecW {                       // chore_mesh_sdf_fwd only: corners b and c (a is in Rec), 1 = has an area / 0 = ab x ac is exactly 0
    float bx, by, bz, cx, cy, cz, area, pad;
};
constexpr int MD_RECW = 8;          // floats per RecW
static_assert(sizeof(Rec) == MD_REC * sizeof(float), "one record is one 64-byte line");
static_assert(sizeof(RecW) == MD_RECW * sizeof(float), "two RecW are one 64-byte line");

// the number of face chunks: a function of the shapes alone (the workspace size and the result's bits depend on it)
__host__ __device__ inline int md_chunks(int B, int N, int F) {
    const long long tiles = (long long)B * ((N + MD_PTS - 1) / MD_PTS);
    long long s = (MD_WANT_GROUPS + tiles - 1) / tiles;
    const int ftiles = (F + MD_TILE - 1) / MD_TILE;
    if (s > ftiles) s = ftiles;
    if (s > MD_MAX_CHUNKS) s = MD_MAX_CHUNKS;
    return s < 1 ? 1 : (int)s;
}
// faces per chunk: whole LDS tiles
__host__ __device__ inline int md_chunk_faces(int F, int S) {
    const int ftiles = (F + MD_TILE - 1) / MD_TILE;
    return ((ftiles + S - 1) / S) * MD_TILE;
}
inline bool md_shape_ok(int B, int N, int V, int F) {
    return B >= 1 && N >= 1 && V >= 1 && F >= 1 && B <= 65535 && (long long)B * N <= (1ll << 30) && (long long)B * F <= (1ll << 26) &&
           (long long)B * V <= (1ll << 28);
}

__device__ __forceinline__ float guarded_recip(double x) {
    if (!(x > 0.0)) return 0.f;
    const float r = (float)(1.0 / x);
    return r < 3.0e38f ? r : 0.f;
}

// The bodies of the three kernels are templates; the __global__ functions below them are the two instantiations, the unsigned
// ones under the names and with the parameters they always had.
template <bool WIND>
__device__ __forceinline__ void record_body(const float* __restrict__ verts, const int* __restrict__ faces, int V, int F,
                                            Rec* __restrict__ rec, RecW* __restrict__ recw) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int b = blockIdx.y;
    const float* vb = verts + (size_t)b * V * 3;
    int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    i0 = min(max(i0, 0), V - 1), i1 = min(max(i1, 0), V - 1), i2 = min(max(i2, 0), V - 1);   // never read outside the mesh
    Rec r;
    r.ax = vb[i0 * 3], r.ay = vb[i0 * 3 + 1], r.az = vb[i0 * 3 + 2];
    r.abx = vb[i1 * 3] - r.ax, r.aby = vb[i1 * 3 + 1] - r.ay, r.abz = vb[i1 * 3 + 2] - r.az;
    r.acx = vb[i2 * 3] - r.ax, r.acy = vb[i2 * 3 + 1] - r.ay, r.acz = vb[i2 * 3 + 2] - r.az;
    const double abx = r.abx, aby = r.aby, abz = r.abz, acx = r.acx, acy = r.acy, acz = r.acz;
    const double bcx = (double)(r.acx - r.abx), bcy = (double)(r.acy - r.aby), bcz = (double)(r.acz - r.abz);   // as the loop forms it
    const double aa = abx * abx + aby * aby + abz * abz, cc = acx * acx + acy * acy + acz * acz;
    const double e = abx * acx + aby * acy + abz * acz;
    r.inv_ab = guarded_recip(aa);
    r.inv_ac = guarded_recip(cc);
    r.inv_bc = guarded_recip(bcx * bcx + bcy * bcy + bcz * bcz);
    const double det = aa * cc - e * e;              // 4 area^2; relative error 1e-16 aa cc in fp64
    float k1 = 0.f, k2 = 0.f, k3 = 0.f;
    if (det > 1e-12 * aa * cc) {
        k1 = (float)(cc / det), k2 = (float)(e / det), k3 = (float)(aa / det);
        if (!(fabsf(k1) < 3.0e38f && fabsf(k2) < 3.0e38f && fabsf(k3) < 3.0e38f)) k1 = k2 = k3 = 0.f;
    }
    r.k1 = k1, r.k2 = k2, r.k3 = k3;
    r.pad = 0.f;
    rec[(size_t)b * F + f] = r;
    if constexpr (WIND) {   // products of fp32 values are exact in fp64: every component is 0 only if ab and ac are exactly parallel
        const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
        RecW w;
        w.bx = vb[i1 * 3], w.by = vb[i1 * 3 + 1], w.bz = vb[i1 * 3 + 2];
        w.cx = vb[i2 * 3], w.cy = vb[i2 * 3 + 1], w.cz = vb[i2 * 3 + 2];
        w.area = (nx != 0.0 || ny != 0.0 || nz != 0.0) ? 1.f : 0.f;
        w.pad = 0.f;
        recw[(size_t)b * F + f] = w;
    }
}
__global__ __launch_bounds__(256) void record_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int V, int F,
                                                     Rec* __restrict__ rec) {
    record_body<false>(verts, faces, V, F, rec, nullptr);
}
__global__ __launch_bounds__(256) void record_kernel_w(const float* __restrict__ verts, const int* __restrict__ faces, int V, int F,
                                                       Rec* __restrict__ rec, RecW* __restrict__ recw) {
    record_body<true>(verts, faces, V, F, rec, recw);
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// squared distance from p to the triangle of `t`; (rx, ry, rz) = p - closest point.  Candidates in a fixed order (edge ab,
// edge ac, edge bc, interior), the first smallest wins.
__device__ __forceinline__ float tri_dist2(const Rec& t, float px, float py, float pz, float& rx, float& ry, float& rz) {
    const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
    const float d1 = fmaf(t.abz, apz, fmaf(t.aby, apy, t.abx * apx));
    const float d2 = fmaf(t.acz, apz, fmaf(t.acy, apy, t.acx * apx));
    // edge ab
    const float t1 = clamp01(d1 * t.inv_ab);
    const float r1x = fmaf(-t1, t.abx, apx), r1y = fmaf(-t1, t.aby, apy), r1z = fmaf(-t1, t.abz, apz);
    const float q1 = fmaf(r1z, r1z, fmaf(r1y, r1y, r1x * r1x));
    // edge ac
    const float t2 = clamp01(d2 * t.inv_ac);
    const float r2x = fmaf(-t2, t.acx, apx), r2y = fmaf(-t2, t.acy, apy), r2z = fmaf(-t2, t.acz, apz);
    const float q2 = fmaf(r2z, r2z, fmaf(r2y, r2y, r2x * r2x));
    // edge bc
    const float bcx = t.acx - t.abx, bcy = t.acy - t.aby, bcz = t.acz - t.abz;
    const float bpx = apx - t.abx, bpy = apy - t.aby, bpz = apz - t.abz;
    const float d3 = fmaf(bcz, bpz, fmaf(bcy, bpy, bcx * bpx));
    const float t3 = clamp01(d3 * t.inv_bc);
    const float r3x = fmaf(-t3, bcx, bpx), r3y = fmaf(-t3, bcy, bpy), r3z = fmaf(-t3, bcz, bpz);
    const float q3 = fmaf(r3z, r3z, fmaf(r3y, r3y, r3x * r3x));
    // interior: a + v ab + w ac with u = 1 - v - w, v, w > 0 is a point of the triangle whatever the rounding of v and w
    const float v = fmaf(t.k1, d1, -(t.k2 * d2)), w = fmaf(t.k3, d2, -(t.k2 * d1));
    const float u = (1.f - v) - w;
    const float r4x = fmaf(-w, t.acx, fmaf(-v, t.abx, apx)), r4y = fmaf(-w, t.acy, fmaf(-v, t.aby, apy)),
                r4z = fmaf(-w, t.acz, fmaf(-v, t.abz, apz));
    const float q4 = fmaf(r4z, r4z, fmaf(r4y, r4y, r4x * r4x));
    float q = q1;
    rx = r1x, ry = r1y, rz = r1z;
    if (q2 < q) q = q2, rx = r2x, ry = r2y, rz = r2z;
    if (q3 < q) q = q3, rx = r3x, ry = r3y, rz = r3z;
    if (fminf(u, fminf(v, w)) > 0.f && q4 < q) q = q4, rx = r4x, ry = r4y, rz = r4z;
    return q;
}

// the same minimum without the foot point (the inner loop)
__device__ __forceinline__ float tri_dist2(const Rec& t, float px, float py, float pz) {
    float rx, ry, rz;
    return tri_dist2(t, px, py, pz, rx, ry, rz);
}

// half the signed solid angle of the triangle seen from p: atan2(determinant, denominator) of van Oosterom & Strackee with a, b, c
// = corners minus p, positive where p sees the back of the triangle (inside an outward-oriented closed mesh the halves add up to
// 2 pi).  Plain products in the cross product: two equal vectors give exactly 0.
__device__ __forceinline__ float tri_half_angle(const Rec& t, const RecW& w, float px, float py, float pz) {
    const float ax = t.ax - px, ay = t.ay - py, az = t.az - pz;
    const float bx = w.bx - px, by = w.by - py, bz = w.bz - pz;
    const float cx = w.cx - px, cy = w.cy - py, cz = w.cz - pz;
    const float nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
    const float det = w.area * (ax * nx + ay * ny + az * nz);
    const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz), lc = sqrtf(cx * cx + cy * cy + cz * cz);
    const float ab = ax * bx + ay * by + az * bz, ac = ax * cx + ay * cy + az * cz, bc = bx * cx + by * cy + bz * cz;
    const float den = la * lb * lc + ab * lc + ac * lb + bc * la;      // the first term is >= +0: a sum of zeros is +0, never -0
    return atan2f(det, den);
}

__device__ __forceinline__ unsigned long long md_key(float d2, int idx) {
    return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned int)idx;
}

template <bool WIND>
__device__ __forceinline__ void dist_body(const float* __restrict__ points, const Rec* __restrict__ rec, int N, int F, int chunk_faces,
                                          unsigned long long* __restrict__ keys, const RecW* __restrict__ recw,
                                          float* __restrict__ wpart) {
    __shared__ f32x4 tile[MD_TILE * (MD_REC + (WIND ? MD_RECW : 0)) / 4];      // WIND: the RecW of the tile behind its Rec
    f32x4* const tilew = tile + MD_TILE * MD_REC / 4;
    const int b = blockIdx.z, s = blockIdx.y;
    const float* pb = points + (size_t)b * N * 3;
    float px[MD_P], py[MD_P], pz[MD_P], best[MD_P];
    float wsum[MD_P];                 // WIND: sum of the half solid angles of this chunk's triangles, in face order
    int bidx[MD_P];
#pragma unroll
    for (int k = 0; k < MD_P; ++k) {
        const int i = min(blockIdx.x * MD_PTS + k * MD_THREADS + (int)threadIdx.x, N - 1);
        px[k] = pb[(size_t)i * 3], py[k] = pb[(size_t)i * 3 + 1], pz[k] = pb[(size_t)i * 3 + 2];
        best[k] = __uint_as_float(0x7f800000u);
        bidx[k] = 0x7fffffff;
        wsum[k] = 0.f;
    }
    const int f0 = s * chunk_faces, f1 = min(F, f0 + chunk_faces);
    const f32x4* src = (const f32x4*)(rec + (size_t)b * F);
    const f32x4* srcw = WIND ? (const f32x4*)(recw + (size_t)b * F) : nullptr;
    for (int base = f0; base < f1; base += MD_TILE) {
        const int n = min(MD_TILE, f1 - base);
        __syncthreads();
        for (int k = threadIdx.x; k < n * (MD_REC / 4); k += MD_THREADS) tile[k] = src[(size_t)base * (MD_REC / 4) + k];
        if constexpr (WIND)
            for (int k = threadIdx.x; k < n * (MD_RECW / 4); k += MD_THREADS) tilew[k] = srcw[(size_t)base * (MD_RECW / 4) + k];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const f32x4 r0 = tile[j * 4], r1 = tile[j * 4 + 1], r2 = tile[j * 4 + 2], r3 = tile[j * 4 + 3];
            Rec t;
            t.ax = r0.x, t.ay = r0.y, t.az = r0.z, t.abx = r0.w;
            t.aby = r1.x, t.abz = r1.y, t.acx = r1.z, t.acy = r1.w;
            t.acz = r2.x, t.inv_ab = r2.y, t.inv_ac = r2.z, t.inv_bc = r2.w;
            t.k1 = r3.x, t.k2 = r3.y, t.k3 = r3.z, t.pad = 0.f;
            RecW w = {};
            if constexpr (WIND) {
                const f32x4 w0 = tilew[j * 2], w1 = tilew[j * 2 + 1];
                w.bx = w0.x, w.by = w0.y, w.bz = w0.z, w.cx = w0.w, w.cy = w1.x, w.cz = w1.y, w.area = w1.z;
            }
#pragma unroll
            for (int k = 0; k < MD_P; ++k) {
                const float q = tri_dist2(t, px[k], py[k], pz[k]);
                if (q < best[k]) best[k] = q, bidx[k] = base + j;     // ascending faces, strict <: the smallest index keeps a tie
                if constexpr (WIND) wsum[k] += tri_half_angle(t, w, px[k], py[k], pz[k]);
            }
        }
    }
    unsigned long long* kout = keys + ((size_t)s * gridDim.z + b) * N;
#pragma unroll
    for (int k = 0; k < MD_P; ++k) {
        const int i = blockIdx.x * MD_PTS + k * MD_THREADS + (int)threadIdx.x;
        if (i < N) kout[i] = md_key(best[k], bidx[k]);
    }
    if constexpr (WIND) {
        float* wout = wpart + ((size_t)s * gridDim.z + b) * N;
#pragma unroll
        for (int k = 0; k < MD_P; ++k) {
            const int i = blockIdx.x * MD_PTS + k * MD_THREADS + (int)threadIdx.x;
            if (i < N) wout[i] = wsum[k];
        }
    }
}
__global__ __launch_bounds__(MD_THREADS) void dist_kernel(const float* __restrict__ points, const Rec* __restrict__ rec, int N, int F,
                                                          int chunk_faces, unsigned long long* __restrict__ keys) {
    dist_body<false>(points, rec, N, F, chunk_faces, keys, nullptr, nullptr);
}
__global__ __launch_bounds__(MD_THREADS) void dist_kernel_w(const float* __restrict__ points, const Rec* __restrict__ rec, int N, int F,
                                                            int chunk_faces, unsigned long long* __restrict__ keys,
                                                            const RecW* __restrict__ recw, float* __restrict__ wpart) {
    dist_body<true>(points, rec, N, F, chunk_faces, keys, recw, wpart);
}

template <bool WIND>
__device__ __forceinline__ void finish_body(const float* __restrict__ points, const Rec* __restrict__ rec,
                                            const unsigned long long* __restrict__ keys, int N, int F, int S, float* __restrict__ dist,
                                            int* __restrict__ face_idx, float* __restrict__ closest, const float* __restrict__ wpart,
                                            float* __restrict__ winding) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int b = blockIdx.y, B = gridDim.y;
    unsigned long long best = keys[(size_t)b * N + i];
    for (int s = 1; s < S; ++s) {
        const unsigned long long k = keys[((size_t)s * B + b) * N + i];
        best = k < best ? k : best;         // squared distances are >= 0: their bit patterns order like the values
    }
    const size_t o = (size_t)b * N + i;
    const int f = min((int)(unsigned int)(best & 0xffffffffu), F - 1);
    dist[o] = sqrtf(__uint_as_float((unsigned int)(best >> 32)));
    if (face_idx) face_idx[o] = f;
    if (closest) {
        const float px = points[o * 3], py = points[o * 3 + 1], pz = points[o * 3 + 2];
        float rx, ry, rz;
        tri_dist2(rec[(size_t)b * F + f], px, py, pz, rx, ry, rz);
        closest[o * 3] = px - rx, closest[o * 3 + 1] = py - ry, closest[o * 3 + 2] = pz - rz;
    }
    if constexpr (WIND) {
        float w = wpart[o];
        for (int s = 1; s < S; ++s) w += wpart[((size_t)s * B + b) * N + i];      // ascending chunks: one order, one result
        winding[o] = w * 0.15915494309189535f;       // sum of half angles / 2 pi = sum of solid angles / 4 pi
    }
}
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ points, const Rec* __restrict__ rec,
                                                     const unsigned long long* __restrict__ keys, int N, int F, int S,
                                                     float* __restrict__ dist, int* __restrict__ face_idx, float* __restrict__ closest) {
    finish_body<false>(points, rec, keys, N, F, S, dist, face_idx, closest, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void finish_kernel_w(const float* __restrict__ points, const Rec* __restrict__ rec,
                                                       const unsigned long long* __restrict__ keys, int N, int F, int S,
                                                       float* __restrict__ dist, int* __restrict__ face_idx, float* __restrict__ closest,
                                                       const float* __restrict__ wpart, float* __restrict__ winding) {
    finish_body<true>(points, rec, keys, N, F, S, dist, face_idx, closest, wpart, winding);
}

__global__ __launch_bounds__(256) void vertex_kernel(const float* __restrict__ points, const float* __restrict__ verts, int N, int V,
                                                     int* __restrict__ vert_idx) {
    __shared__ float tile[MD_VTILE * 3];
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x, ic = min(i, N - 1);
    const float* pb = points + ((size_t)b * N + ic) * 3;
    const float px = pb[0], py = pb[1], pz = pb[2];
    const float* vb = verts + (size_t)b * V * 3;
    float best = __uint_as_float(0x7f800000u);
    int bi = 0;
    for (int base = 0; base < V; base += MD_VTILE) {
        const int n = min(MD_VTILE, V - base);
        __syncthreads();
        for (int k = threadIdx.x; k < n * 3; k += 256) tile[k] = vb[(size_t)base * 3 + k];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float dx = px - tile[j * 3], dy = py - tile[j * 3 + 1], dz = pz - tile[j * 3 + 2];
            const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (d < best) best = d, bi = base + j;
        }
    }
    if (i < N) vert_idx[(size_t)b * N + i] = bi;
}

// workspace of both entry points: Rec [B*F] | keys [S*B*N] | with `wind` also: winding partials float [S*B*N] | RecW [B*F]
struct MdWs { Rec* rec; unsigned long long* keys; float* wpart; RecW* recw; size_t bytes; };
MdWs md_ws(void* base, bool wind, int B, int N, int F) {
    const size_t BF = (size_t)B * F, SBN = (size_t)md_chunks(B, N, F) * B * N;
    WsCarver c(base);
    return {c.take<Rec>(BF), c.take<unsigned long long>(SBN), wind ? c.take<float>(SBN) : nullptr,
            wind ? c.take<RecW>(BF) : nullptr, c.bytes};
}

// the three launches (+ the nearest-vertex one) of both entry points; `wpart` / `winding` are read by the WIND kernels only
template <bool WIND>
int md_run(chore_handle* h, const char* who, const float* points, const float* verts, const int* faces, int B, int N, int V, int F,
           float* dist, int* face_idx, float* closest, int* vert_idx, float* winding, void* workspace, chore_stream_t stream) {
    if (!md_shape_ok(B, N, V, F)) CHORE_FAIL(h, CHORE_EINVAL, "%s: unsupported shape B=%d N=%d V=%d F=%d", who, B, N, V, F);
    if (!points || !verts || !faces || !dist || !workspace || (WIND && !winding)) CHORE_FAIL(h, CHORE_EINVAL, "%s: bad argument", who);
    hipStream_t s = (hipStream_t)stream;
    const int S = md_chunks(B, N, F);
    const MdWs w = md_ws(workspace, WIND, B, N, F);
    const dim3 grec((F + 255) / 256, B), gdist((N + MD_PTS - 1) / MD_PTS, S, B), gfin((N + 255) / 256, B);
    if constexpr (WIND) {
        hipLaunchKernelGGL(record_kernel_w, grec, dim3(256), 0, s, verts, faces, V, F, w.rec, w.recw);
        CHORE_LAUNCH_CHECK(h, s);
        hipLaunchKernelGGL(dist_kernel_w, gdist, dim3(MD_THREADS), 0, s, points, (const Rec*)w.rec, N, F, md_chunk_faces(F, S), w.keys,
                           (const RecW*)w.recw, w.wpart);
        CHORE_LAUNCH_CHECK(h, s);
        hipLaunchKernelGGL(finish_kernel_w, gfin, dim3(256), 0, s, points, (const Rec*)w.rec, (const unsigned long long*)w.keys, N, F, S, dist,
                           face_idx, closest, (const float*)w.wpart, winding);
        CHORE_LAUNCH_CHECK(h, s);
    } else {
        hipLaunchKernelGGL(record_kernel, grec, dim3(256), 0, s, verts, faces, V, F, w.rec);
        CHORE_LAUNCH_CHECK(h, s);
        hipLaunchKernelGGL(dist_kernel, gdist, dim3(MD_THREADS), 0, s, points, (const Rec*)w.rec, N, F, md_chunk_faces(F, S), w.keys);
        CHORE_LAUNCH_CHECK(h, s);
        hipLaunchKernelGGL(finish_kernel, gfin, dim3(256), 0, s, points, (const Rec*)w.rec, (const unsigned long long*)w.keys, N, F, S, dist,
                           face_idx, closest);
        CHORE_LAUNCH_CHECK(h, s);
    }
    if (vert_idx) {
        hipLaunchKernelGGL(vertex_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, points, verts, N, V, vert_idx);
        CHORE_LAUNCH_CHECK(h, s);
    }
    return CHORE_OK;
}

}  // namespace

extern "C" {

size_t chore_mesh_dist_workspace_bytes(int B, int N, int V, int F) { return md_shape_ok(B, N, V, F) ? md_ws(nullptr, false, B, N, F).bytes : 0; }

int chore_mesh_dist_fwd(chore_handle* h, const float* points, const float* verts, const int* faces, int B, int N, int V, int F,
                        float* dist, int* face_idx, float* closest, int* vert_idx, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    return md_run<false>(h, "chore_mesh_dist_fwd", points, verts, faces, B, N, V, F, dist, face_idx, closest, vert_idx, nullptr, workspace,
                         stream);
}

// the unsigned call's workspace + one float per (chunk, image, point) + one RecW per (image, face)
size_t chore_mesh_sdf_workspace_bytes(int B, int N, int V, int F) { return md_shape_ok(B, N, V, F) ? md_ws(nullptr, true, B, N, F).bytes : 0; }

int chore_mesh_sdf_fwd(chore_handle* h, const float* points, const float* verts, const int* faces, int B, int N, int V, int F,
                       float* dist, int* face_idx, float* closest, int* vert_idx, float* winding, void* workspace,
                       chore_stream_t stream) {
    CHORE_ENTER(h);
    return md_run<true>(h, "chore_mesh_sdf_fwd", points, verts, faces, B, N, V, F, dist, face_idx, closest, vert_idx, winding, workspace,
                        stream);
}

}  // extern "C"
