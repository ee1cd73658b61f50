// mesh_dist_bwd.hip -- the gradient of the exact point-to-mesh distance (mesh_dist.hip) with respect to the query points and the
// mesh vertices, fp32, gfx950.
//
// For a point p with winning triangle (a0, a1, a2), closest point c = sum_k b_k a_k (b_k >= 0, sum b_k = 1) and d = |p - c| > 0:
//   dd/dp = (p - c) / d,   dd/da_k = -b_k (p - c) / d      (interior, edge and vertex regions alike: d is a minimum over b)
// The forward's saved winner (face_idx) and dist are the input; the winner is not searched for again.
//
//   point_kernel    one thread per (image, point).  The closest point of p on the winning triangle is found again in fp64 by
//                   the triangle's Voronoi regions: its barycentric coordinates b (a point beyond a corner gives that corner
//                   the weight 1 and the others exactly 0; one beyond an edge gives the opposite corner exactly 0), clamped to
//                   [0, 1] with b_0 = 1 - b_1 - b_2, and r = p - c.  A triangle without an area (recognised as record_kernel
//                   of the forward does) is the segment or point it degenerates to: the weights of the foot point nearest to p
//                   on its three edges.  Finite and summing to 1 in every case.  u = g r / |r| (0 where dist == 0) -> dpoints,
//                   and, when dverts is wanted, one record per point: the three vertex ids of its triangle (16 bytes) and u
//                   with b (32 bytes).  The forward's fp32 `closest` is not read: see the note at r below.
//   gather_kernel   grid (vertex tiles, point chunks, B): every thread owns ONE vertex and keeps its three sums in registers.
//                   The chunk's records stream through LDS in tiles of MB_TILE; the ids are read at wave-uniform addresses
//                   (broadcast) and compared with the thread's vertex, the values only on a match.  Ascending points, corners
//                   0, 1, 2 of a point in that order: one order, one result -- no atomics anywhere.
//   finish_kernel   adds the chunks' partial sums in ascending chunk order (not launched when there is one chunk: gather_kernel
//                   then writes dverts itself).
// The number of chunks depends on the shapes alone (mb_chunks), so the bits depend on the shapes and the inputs alone.
#include "common.h"

namespace {

constexpr int MB_THREADS = 256;                  // threads of every kernel; vertices per workgroup of gather_kernel
constexpr int MB_TILE = 256;                     // point records per LDS tile (4 KiB of ids + 8 KiB of values)
constexpr int MB_WANT_GROUPS = 2048;             // workgroups the split over point chunks aims for (8 per CU on 256 CUs)
constexpr int MB_MAX_CHUNKS = 64;

struct RecId {                                   // the three corners of the point's triangle, clamped into [0, V)
    int i0, i1, i2, pad;
};
struct RecVal {                                  // u = g (p - c) / dist and the barycentric coordinates of c
    float ux, uy, uz, b0, b1, b2, pad0, pad1;
};
static_assert(sizeof(RecId) == 16 && sizeof(RecVal) == 32, "one id record is one 16-byte load, one value record two");

// the number of point chunks: a function of the shapes alone (the workspace size and the result's bits depend on it)
__host__ __device__ inline int mb_chunks(int B, int N, int V) {
    const long long tiles = (long long)B * ((V + MB_THREADS - 1) / MB_THREADS);
    long long s = (MB_WANT_GROUPS + tiles - 1) / tiles;
    const int ptiles = (N + MB_TILE - 1) / MB_TILE;
    if (s > ptiles) s = ptiles;
    if (s > MB_MAX_CHUNKS) s = MB_MAX_CHUNKS;
    return s < 1 ? 1 : (int)s;
}
// points per chunk: whole LDS tiles
__host__ __device__ inline int mb_chunk_points(int N, int S) {
    const int ptiles = (N + MB_TILE - 1) / MB_TILE;
    return ((ptiles + S - 1) / S) * MB_TILE;
}
inline bool mb_shape_ok(int B, int N, int V, int F) {
    return B >= 1 && N >= 1 && V >= 1 && F >= 1 && B <= 65535 && (long long)B * N <= (1ll << 26) && (long long)B * F <= (1ll << 26) &&
           (long long)B * V <= (1ll << 26);
}

__device__ __forceinline__ double clamp01d(double x) { return fmin(fmax(x, 0.0), 1.0); }

// the foot point of q on the segment a + t e, t in [0, 1] (a segment of length 0: t = 0): t and the squared distance to it
__device__ __forceinline__ double seg_foot(double qx, double qy, double qz, double ex, double ey, double ez, double& t) {
    const double ee = ex * ex + ey * ey + ez * ez;
    t = ee > 0.0 ? clamp01d((qx * ex + qy * ey + qz * ez) / ee) : 0.0;
    const double rx = qx - t * ex, ry = qy - t * ey, rz = qz - t * ez;
    return rx * rx + ry * ry + rz * rz;
}

__global__ __launch_bounds__(MB_THREADS) void point_kernel(const float* __restrict__ points, const float* __restrict__ verts,
                                                           const int* __restrict__ faces, const int* __restrict__ face_idx,
                                                           const float* __restrict__ dist,
                                                           const float* __restrict__ g_dist, int N, int V, int F,
                                                           float* __restrict__ dpoints, RecId* __restrict__ ids,
                                                           RecVal* __restrict__ vals) {
    const int i = blockIdx.x * MB_THREADS + threadIdx.x;
    if (i >= N) return;
    const int b = blockIdx.y;
    const size_t o = (size_t)b * N + i;
    const float d = dist[o], g = g_dist[o];
    const float px = points[o * 3], py = points[o * 3 + 1], pz = points[o * 3 + 2];
    const int f = min(max(face_idx[o], 0), F - 1);
    RecId r;
    r.i0 = min(max(faces[f * 3], 0), V - 1), r.i1 = min(max(faces[f * 3 + 1], 0), V - 1), r.i2 = min(max(faces[f * 3 + 2], 0), V - 1);
    r.pad = 0;
    const float* vt = verts + (size_t)b * V * 3;
    const double ax = vt[r.i0 * 3], ay = vt[r.i0 * 3 + 1], az = vt[r.i0 * 3 + 2];
    const double abx = vt[r.i1 * 3] - ax, aby = vt[r.i1 * 3 + 1] - ay, abz = vt[r.i1 * 3 + 2] - az;
    const double acx = vt[r.i2 * 3] - ax, acy = vt[r.i2 * 3 + 1] - ay, acz = vt[r.i2 * 3 + 2] - az;
    const double qx = (double)px - ax, qy = (double)py - ay, qz = (double)pz - az;
    const double aa = abx * abx + aby * aby + abz * abz, cc = acx * acx + acy * acy + acz * acz;
    const double e = abx * acx + aby * acy + abz * acz;
    const double det = aa * cc - e * e;              // 4 area^2
    double b1, b2;
    if (det > 1e-12 * aa * cc) {                     // the Voronoi regions of the triangle (Ericson, Real-Time Collision Detection 5.1.5)
        const double d1 = abx * qx + aby * qy + abz * qz, d2 = acx * qx + acy * qy + acz * qz;
        const double d3 = d1 - aa, d4 = d2 - e;      // ab.bp, ac.bp
        const double d5 = d1 - e, d6 = d2 - cc;      // ab.cp, ac.cp
        const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        if (d1 <= 0.0 && d2 <= 0.0) b1 = 0.0, b2 = 0.0;                                   // corner a
        else if (d3 >= 0.0 && d4 <= d3) b1 = 1.0, b2 = 0.0;                               // corner b
        else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) b1 = d1 / (d1 - d3), b2 = 0.0;      // edge ab
        else if (d6 >= 0.0 && d5 <= d6) b1 = 0.0, b2 = 1.0;                               // corner c
        else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) b1 = 0.0, b2 = d2 / (d2 - d6);      // edge ac
        else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {                         // edge bc
            b2 = (d4 - d3) / ((d4 - d3) + (d5 - d6));
            b1 = 1.0 - b2;
        } else {                                                                          // interior
            const double den = va + vb + vc;
            b1 = vb / den, b2 = vc / den;
        }
        b1 = clamp01d(b1);
        b2 = fmin(clamp01d(b2), 1.0 - b1);
    } else {                                         // a segment or a point: the nearest of the three edges' foot points
        double t1, t2, t3;
        const double q1 = seg_foot(qx, qy, qz, abx, aby, abz, t1);
        const double q2 = seg_foot(qx, qy, qz, acx, acy, acz, t2);
        const double q3 = seg_foot(qx - abx, qy - aby, qz - abz, acx - abx, acy - aby, acz - abz, t3);
        b1 = t1, b2 = 0.0;
        double q = q1;
        if (q2 < q) q = q2, b1 = 0.0, b2 = t2;
        if (q3 < q) b1 = 1.0 - t3, b2 = t3;
    }
    // r = p - c with c = a + b1 ab + b2 ac, in fp64: the direction is then good to the rounding of the OUTPUT.  (p - `closest`
    // in fp32 carries the rounding of the stored closest point, eps |c|, into the direction as eps |c| / dist: measured 1.7e-4
    // on the box of 1 728 faces, z up to 2.6, 33 times the float32 restatement's own error there.)
    const double rx = qx - b1 * abx - b2 * acx, ry = qy - b1 * aby - b2 * acy, rz = qz - b1 * abz - b2 * acz;
    const double rr = sqrt(rx * rx + ry * ry + rz * rz);
    float ux = 0.f, uy = 0.f, uz = 0.f;
    if (d > 0.f && rr > 0.0) ux = (float)(g * (rx / rr)), uy = (float)(g * (ry / rr)), uz = (float)(g * (rz / rr));
    if (dpoints) dpoints[o * 3] = ux, dpoints[o * 3 + 1] = uy, dpoints[o * 3 + 2] = uz;
    if (!ids) return;
    RecVal w;
    w.ux = ux, w.uy = uy, w.uz = uz;
    w.b1 = (float)b1, w.b2 = (float)b2;
    w.b0 = (float)fmax((1.0 - b1) - b2, 0.0);
    w.pad0 = w.pad1 = 0.f;
    ids[o] = r;
    vals[o] = w;
}

__global__ __launch_bounds__(MB_THREADS) void gather_kernel(const RecId* __restrict__ ids, const RecVal* __restrict__ vals, int N, int V,
                                                            int chunk_points, float* __restrict__ out) {
    __shared__ u32x4 tid_[MB_TILE];
    __shared__ f32x4 tval[MB_TILE * 2];
    const int b = blockIdx.z, s = blockIdx.y;
    const int v = blockIdx.x * MB_THREADS + threadIdx.x;
    const int n0 = min(N, s * chunk_points), n1 = min(N, n0 + chunk_points);
    const u32x4* src_i = (const u32x4*)(ids + (size_t)b * N);
    const f32x4* src_v = (const f32x4*)(vals + (size_t)b * N);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int base = n0; base < n1; base += MB_TILE) {
        const int n = min(MB_TILE, n1 - base);
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += MB_THREADS) tid_[k] = src_i[(size_t)base + k];
        for (int k = threadIdx.x; k < n * 2; k += MB_THREADS) tval[k] = src_v[(size_t)base * 2 + k];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const u32x4 q = tid_[j];
            const bool m0 = (int)q.x == v, m1 = (int)q.y == v, m2 = (int)q.z == v;
            if (m0 | m1 | m2) {                      // rare: a vertex is a corner of few points' triangles
                const f32x4 a = tval[j * 2], c = tval[j * 2 + 1];      // ux uy uz b0 | b1 b2 - -
                if (m0) sx += -(a.w * a.x), sy += -(a.w * a.y), sz += -(a.w * a.z);
                if (m1) sx += -(c.x * a.x), sy += -(c.x * a.y), sz += -(c.x * a.z);
                if (m2) sx += -(c.y * a.x), sy += -(c.y * a.y), sz += -(c.y * a.z);
            }
        }
    }
    if (v < V) {
        float* o = out + (((size_t)s * gridDim.z + b) * V + v) * 3;
        o[0] = sx, o[1] = sy, o[2] = sz;
    }
}

__global__ __launch_bounds__(MB_THREADS) void finish_kernel(const float* __restrict__ part, int V3, int S, float* __restrict__ dverts) {
    const int e = blockIdx.x * MB_THREADS + threadIdx.x;
    if (e >= V3) return;
    const int b = blockIdx.y, B = gridDim.y;
    float a = part[(size_t)b * V3 + e];
    for (int s = 1; s < S; ++s) a += part[((size_t)s * B + b) * V3 + e];      // ascending chunks: one order, one result
    dverts[(size_t)b * V3 + e] = a;
}

// workspace: one id and one value record per (image, point) | one partial sum per (chunk, image, vertex)
struct MbWs { RecId* ids; RecVal* vals; float* part; size_t bytes; };
MbWs mb_ws(void* base, int B, int N, int V) {
    WsCarver c(base);
    return {c.take<RecId>((size_t)B * N), c.take<RecVal>((size_t)B * N), c.take<float>((size_t)mb_chunks(B, N, V) * B * V * 3), c.bytes};
}

}  // namespace

extern "C" {

size_t chore_mesh_dist_bwd_workspace_bytes(int B, int N, int V, int F) { return mb_shape_ok(B, N, V, F) ? mb_ws(nullptr, B, N, V).bytes : 0; }

int chore_mesh_dist_bwd(chore_handle* h, const float* points, const float* verts, const int* faces, const int* face_idx,
                        const float* closest, const float* dist, const float* g_dist, int B, int N, int V, int F, float* dpoints,
                        float* dverts, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!mb_shape_ok(B, N, V, F)) CHORE_FAIL(h, CHORE_EINVAL, "chore_mesh_dist_bwd: unsupported shape B=%d N=%d V=%d F=%d", B, N, V, F);
    if (!points || !verts || !faces || !face_idx || !dist || !g_dist || !workspace)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_mesh_dist_bwd: bad argument");
    if (!dpoints && !dverts) return CHORE_OK;
    hipStream_t s = (hipStream_t)stream;
    const MbWs w = mb_ws(workspace, B, N, V);
    hipLaunchKernelGGL(point_kernel, dim3((N + MB_THREADS - 1) / MB_THREADS, B), dim3(MB_THREADS), 0, s, points, verts, faces, face_idx,
                       dist, g_dist, N, V, F, dpoints, dverts ? w.ids : (RecId*)nullptr, dverts ? w.vals : (RecVal*)nullptr);
    CHORE_LAUNCH_CHECK(h, s);
    if (!dverts) return CHORE_OK;
    const int S = mb_chunks(B, N, V);
    hipLaunchKernelGGL(gather_kernel, dim3((V + MB_THREADS - 1) / MB_THREADS, S, B), dim3(MB_THREADS), 0, s, (const RecId*)w.ids,
                       (const RecVal*)w.vals, N, V, mb_chunk_points(N, S), S == 1 ? dverts : w.part);
    CHORE_LAUNCH_CHECK(h, s);
    if (S > 1) {
        hipLaunchKernelGGL(finish_kernel, dim3((V * 3 + MB_THREADS - 1) / MB_THREADS, B), dim3(MB_THREADS), 0, s, (const float*)w.part, V * 3,
                           S, dverts);
        CHORE_LAUNCH_CHECK(h, s);
    }
    return CHORE_OK;
}

}  // extern "C"
