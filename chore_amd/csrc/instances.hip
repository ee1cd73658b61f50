// instances.hip -- instance masks and visibility of meshes: which group of faces owns a sample, and which groups would
// cover it if the others were not there.  Forward only.
//
// Replaces neural_renderer's mode='visibility' (external/neural_renderer/neural_renderer/renderer.py:79-117,
// visibility.py:12-34, the atomicMax on face_visibility in forward_face_index_map, cuda/rasterize_cuda_kernel.cu:200-205)
// and makes the three masks BEHAVE ships per frame (the person, the object as seen, the object alone) from the meshes.
// The rule is chore_instances_fwd's in include/chore_hip.h.  Organisation:
//   * the clear kernel (raster_store.h; the bin counters and the two count outputs = 0), the setup kernel (raster_common.h), the
//     bins and the walk (render_common.h) are the family's: one walk of a tile over its bin's list, the
//     callback sees every face that hits a sample.  Per sample the lane keeps the (zp, f) minimum with the winner's group, and
//     an 8-bit mask of the groups met.  Three chore_render_fwd calls (all meshes, each mesh alone) would walk the same bins
//     three times and shade every sample on top.
//   * the masks are resolved and stored by the owning lane, like chore_render_fwd's alpha.  They are small integers times
//     1 / ssaa^2, so they are exact.
//   * the counts are integers throughout.  group_samples: a lane packs its two counts of a group into one word (at most 4
//     each), a butterfly sums the wave's (at most 256 each), LDS the four waves', and one thread per (group, kind) adds the
//     workgroup's total.  face_samples: a lane merges the equal winners among its samples, then the wave merges equal faces
//     (a leader's face is broadcast, the lanes that hold it sum their counts, the leader adds once), so a face that fills the
//     tile costs one add per wave and sample slot and not 256.  Integer sums do not depend on the order of arrival: every
//     output is bit-equal from call to call and under graph replay.
#include "render_common.h"

namespace {

constexpr int INST_MAX_GROUPS = 8;

template <int SS>
__global__ __launch_bounds__(256) void instances_tile_kernel(const TriSetup* __restrict__ ts, const int* __restrict__ count,
                                                             const int* __restrict__ list, const int* __restrict__ face_group,
                                                             int F, int G, int size, float near, float far,
                                                             float* __restrict__ visible, float* __restrict__ full,
                                                             int* __restrict__ face_samples, int* __restrict__ group_samples,
                                                             int* __restrict__ sample_face_index) {
    constexpr int NS = SS * SS;
    __shared__ RbShared sh;
    __shared__ int gsum[4][INST_MAX_GROUPS];               // per wave and group: visible | full << 16
    const int b = blockIdx.z;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int* grp = face_group ? face_group + (size_t)b * F : nullptr;
    int px, py;
    bool inside;
    float zb[NS];
    int best[NS], bg[NS];                                  // the winner and its group (-1 = none / an occluder)
    unsigned cover[NS];                                    // bit g: a candidate of group g
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        zb[s] = far; best[s] = -1; bg[s] = -1; cover[s] = 0u;
    }
    rb_walk_hits<SS>(sh, ts, count, list, F, size, near, far, px, py, inside, [&](int s, int id, float zp, const float*) {
        if (!(zp == zp)) return;                           // raster_hit lets a NaN depth through; it never wins in rb_walk
        const int g = grp ? grp[id] : 0;
        const bool member = (unsigned)g < (unsigned)G;
        if (member) cover[s] |= 1u << g;
        // rb_walk's rule: smallest depth, then smallest index
        if (zp < zb[s] || (zp == zb[s] && best[s] >= 0 && id < best[s])) {
            zb[s] = zp; best[s] = id; bg[s] = member ? g : -1;
        }
    });
    // a lane outside the image met no face: it stores nothing and adds zeros below

    const int row = size - 1 - py;                          // chore_render_fwd's flip
    const size_t plane = (size_t)size * size, o = (size_t)row * size + px;
    constexpr float inv_ns = 1.f / NS;
#pragma unroll
    for (int g = 0; g < INST_MAX_GROUPS; ++g) {
        if (g >= G) break;                                  // G is uniform
        int nv = 0, nf = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            nv += bg[s] == g ? 1 : 0;
            nf += (int)((cover[s] >> g) & 1u);
        }
        if (inside) {
            if (visible) visible[((size_t)b * G + g) * plane + o] = (float)nv * inv_ns;
            if (full) full[((size_t)b * G + g) * plane + o] = (float)nf * inv_ns;
        }
        int packed = nv | (nf << 16);                       // <= 4 each; the wave's sums are <= 256 each
#pragma unroll
        for (int d = 32; d; d >>= 1) packed += __shfl_xor(packed, d);
        if (ln == 0) gsum[wv][g] = packed;
    }
    if (inside && sample_face_index) raster_store_sample_ids<SS>(sample_face_index, b, px, py, size, best);
    __syncthreads();
    if (group_samples && (int)threadIdx.x < 2 * G) {
        const int g = threadIdx.x >> 1, kind = threadIdx.x & 1;
        int n = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) n += (gsum[q][g] >> (16 * kind)) & 0xffff;
        if (n) atomicAdd(&group_samples[((size_t)b * G + g) * 2 + kind], n);
    }

    if (face_samples) {
        int* fsb = face_samples + (size_t)b * F;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            // this lane's distinct winners: sample s speaks for the later samples with the same face
            int f = best[s], c = 0;
#pragma unroll
            for (int q = 0; q < s; ++q)
                if (best[q] == f) f = -1;
#pragma unroll
            for (int q = s; q < NS; ++q) c += best[q] == f ? 1 : 0;
            // the wave's distinct faces, one add each (every lane of the wave is here: nobody has returned)
            unsigned long long todo = __ballot(f >= 0);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int lf = __shfl(f, leader);
                const bool mine = f == lf;
                int n = mine ? c : 0;
#pragma unroll
                for (int d = 32; d; d >>= 1) n += __shfl_xor(n, d);
                if (ln == leader) atomicAdd(&fsb[lf], n);
                todo &= ~__ballot(mine);
            }
        }
    }
}

}  // namespace

extern "C" size_t chore_instances_workspace_bytes(int B, int F, int G, int size, int ssaa) {
    if (G < 1 || G > INST_MAX_GROUPS || !render_shape_ok(B, F, 2, size, ssaa)) return 0;
    return render_ws_bytes(B, F, size, ssaa);
}

extern "C" int chore_instances_fwd(chore_handle* h, const float* tri, const int* face_group, int B, int F, int G, int size,
                                   int ssaa, float near_z, float far_z, float* visible, float* full, int* face_samples,
                                   int* group_samples, int* sample_face_index, void* workspace, chore_stream_t stream) {
    CHORE_ENTER(h);
    if (!tri || !workspace) CHORE_FAIL(h, CHORE_EINVAL, "chore_instances_fwd: null argument");
    if (!visible && !full && !face_samples && !group_samples && !sample_face_index)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_instances_fwd: all outputs are NULL");
    if (ssaa != 1 && ssaa != 2) CHORE_FAIL(h, CHORE_EINVAL, "chore_instances_fwd: ssaa must be 1 or 2, got %d", ssaa);
    if (G < 1 || G > INST_MAX_GROUPS)
        CHORE_FAIL(h, CHORE_EINVAL, "chore_instances_fwd: G must be 1..%d, got %d", INST_MAX_GROUPS, G);
    if (!render_shape_ok(B, F, 2, size, ssaa))
        CHORE_FAIL(h, CHORE_EINVAL, "chore_instances_fwd: bad sizes B=%d F=%d size=%d ssaa=%d", B, F, size, ssaa);
    hipStream_t s = (hipStream_t)stream;
    const int S = size * ssaa, nb = rb_bins(S);
    WsCarver c(workspace);
    const RenderWs w = render_ws(c, B, F, S);
    // the bin counters and the two count outputs = 0 in one grid, no keys; a NULL output has n = 0
    const size_t ncount = (size_t)B * nb * nb, nface = face_samples ? (size_t)B * F : 0, ngroup = group_samples ? (size_t)B * G * 2 : 0;
    const size_t nclear = ncount > nface ? (ncount > ngroup ? ncount : ngroup) : (nface > ngroup ? nface : ngroup);
    raster_clear(s, nclear, nullptr, 0, w.count, ncount, face_samples, nface, group_samples, ngroup);
    CHORE_LAUNCH_CHECK(h, s);
    raster_setup(s, tri, B, F, S, w.ts, w.count, w.list);
    CHORE_LAUNCH_CHECK(h, s);
    raster_dispatch_ssaa(ssaa, [&](auto ss) {
        hipLaunchKernelGGL(instances_tile_kernel<decltype(ss)::value>, rb_tile_grid(size, B), dim3(256), 0, s, w.ts, w.count, w.list,
                           face_group, F, G, size, near_z, far_z, visible, full, face_samples, group_samples, sample_face_index);
    });
    CHORE_LAUNCH_CHECK(h, s);
    return CHORE_OK;
}
