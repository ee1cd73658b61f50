"""CPU: the coverage table of tests/test_gpu_mesh_terms.py (mesh_term_cases.COVERAGE) names every entry point of the collision and
silhouette families of chore_amd/_lib.py and include/chore_hip.h, every case family is run by a GPU test, the case counts are pinned
and the constants the shapes were chosen around are the ones in csrc/collision.hip and csrc/silhouette.hip: a changed tile, chunk,
grid or capacity fails here, before anyone reaches a GPU.  Also here, because they need no GPU: tests/collision_ref.py against
oracle/collision.py, and every condition the cases must meet on the references alone."""
import os
import re

import numpy as np

import collision_ref as cr
import mesh_term_cases as mc
from conftest import REPO
from oracle import collision as oc
from oracle import silhouette as osil

CSRC = os.path.join(REPO, "chore_amd", "csrc")


def _src(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_table_names_exactly_the_entry_points():
    text = open(os.path.join(REPO, "chore_amd", "_lib.py")).read()
    names = set(re.findall(r'^\s*"(chore_\w+)"\s*:\s*\(', text, re.M))
    want = {n for n in names if n.startswith(mc.FAMILIES)}
    assert len(want) == 8, sorted(want)
    assert set(mc.COVERAGE) == want, (sorted(want - set(mc.COVERAGE)), sorted(set(mc.COVERAGE) - want))
    header = open(os.path.join(REPO, "include", "chore_hip.h")).read()
    declared = {n for n in re.findall(r"\b(chore_\w+)\(", header) if n.startswith(mc.FAMILIES)}
    assert declared == want, sorted(declared ^ want)
    every = {c["id"] for cs in mc.CASES.values() for c in cs}
    assert len(every) == sum(len(cs) for cs in mc.CASES.values()), "duplicate case ids"
    used = set()
    for name, row in mc.COVERAGE.items():
        assert row and set(row) <= every, name
        used |= set(row)
    assert used == every, sorted(every - used)


def test_every_case_family_is_run_by_a_gpu_test():
    text = open(os.path.join(REPO, "tests", "test_gpu_mesh_terms.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    run = re.findall(r'@pytest\.mark\.parametrize\("case", mc\.CASES\["(\w+)"\], ids=mc\.ids\("(\w+)"\)\)\ndef (test_\w+)\(case\):', text)
    assert all(a == b for a, b, _ in run), run
    assert sorted(a for a, _, _ in run) == sorted(mc.CASES), (run, sorted(mc.CASES))


def test_the_table_holds_the_shapes_it_was_asked_for():
    C, K = mc.CASES, mc.CONSTANTS
    assert {k: len(v) for k, v in C.items()} == {"coll_tiles": 12, "coll_rounds": 1, "coll_meshes": 2, "coll_order": 3, "coll_zero_area": 1,
                                                 "coll_caps": 2, "sil_fwd": 6, "sil_bwd": 2, "sil_project": 13}
    ct = K["CT"]
    assert {(c["F"], c["B"]) for c in C["coll_tiles"]} == {(F, B) for F in (1, 2, ct - 1, ct, ct + 1, 2 * ct + 1) for B in (1, 3)}
    assert {c["of"] for c in C["coll_order"]} == {"coll_tiles.F257.B3", "coll_meshes.spheres", C["coll_rounds"][0]["id"]}
    assert [(c["m"], c["counts"]) for c in C["coll_caps"]] == [(64, [2048, 0, 2048]), (100, [2624, 1104, 6272])]
    assert [(c["L"], c["size"], c["B"]) for c in C["sil_fwd"]] == [(1, 15, 1), (255, 16, 1), (256, 17, 3), (257, 50, 1), (600, 50, 3), (600, 17, 1)]
    assert [(c["L"], c["size"], c["B"]) for c in C["sil_bwd"]] == [(256, 17, 3), (257, 50, 1)]
    ch, px = K["CHUNK"], K["TILE_PX"]
    assert {c["L"] for c in C["sil_fwd"]} >= {1, ch - 1, ch, ch + 1} and max(c["L"] for c in C["sil_fwd"]) > 2 * ch
    assert sum(c["size"] % px != 0 for c in C["sil_fwd"]) >= 4 and any(c["size"] < px for c in C["sil_fwd"]) and any(c["size"] > 3 * px for c in C["sil_fwd"])
    P = C["sil_project"]
    blk = K["PROJ_BLOCK"]
    assert {(c["V"], c["F"]) for c in P} == {(3, 1), (blk - 1, blk // 2 - 1), (blk, blk // 2), (blk + 1, blk // 2 + 1), (600, 1100)}
    assert len(P) >= 12 and 600 > 2 * blk and 2 * 1100 > 8 * blk
    for key, vals in (("B", {1, 3}), ("dist", {0, 1}), ("orig", {1.0, 2.0}), ("bcast", {0, 1})):
        assert {c[key] for c in P} == vals, key
    assert {(c["V"], c["F"]) for c in P if c["dist"]} == {(c["V"], c["F"]) for c in P}          # every (V, F) with distortion on
    assert any(c["B"] == 3 and not c["bcast"] for c in P)                                          # three different cameras
    for c in P:
        d = mc.project_inputs(c["id"])
        assert d["cam_R"].shape[0] == (1 if c["bcast"] else c["B"])
        assert c["bcast"] or c["B"] == 1 or not np.array_equal(d["cam_R"][0], d["cam_R"][1])
        assert (d["dist5"] is None) == (not c["dist"]) and (d["dist5"] is None or tuple(d["dist5"]) == tuple(np.float32(mc.DIST5)))


def test_constants_are_the_sources():
    K = mc.CONSTANTS
    const = lambda src, name: int(re.search(r"constexpr int (?:\w+ = \d+, )*%s = (\d+)" % name, src).group(1))      # noqa: E731
    co = _src("collision.hip")
    assert const(co, "CT") == K["CT"]
    assert "inline int coll_cand_cap(int F) { return F * %d + %d; }" % K["CAND_CAP"] in co
    assert "inline int coll_pair_cap(int F) { return F * %d + %d; }" % K["PAIR_CAP"] in co
    assert "coll_broad_kernel, dim3(%d, B), dim3(256)" % K["BROAD_GRID"] in co and "pi += gridDim.x" in co
    assert "coll_narrow_kernel, dim3(256, B), dim3(256)" in co and K["NARROW_THREADS"] == 256 * 256
    assert "coll_loss_kernel, dim3(256, B), dim3(64)" in co and K["LOSS_THREADS"] == 256 * 64
    assert co.count("c += gridDim.x * blockDim.x") == 2
    assert "coll_tilepairs_kernel, dim3((nt * (nt + 1) / 2 + 255) / 256, B), dim3(256)" in co and "p = blockIdx.x * 256 + threadIdx.x" in co
    assert K["TILEPAIR_BLOCK"] == 256
    assert "constexpr double FX_LOSS = 4294967296.0;" in co and "constexpr double FX_GRAD = 16777216.0;" in co      # 2^32, 2^24: the bounds
    assert "if (base < (unsigned)w.cand_cap)" in co and "if (k < (unsigned)w.pair_cap)" in co
    si = _src("silhouette.hip")
    assert const(si, "CHUNK") == K["CHUNK"] and const(si, "TILE_PX") == K["TILE_PX"]
    assert "sil_project_fwd_kernel, dim3((2 * F + 255) / 256, B), dim3(256)" in si and "f2 = blockIdx.x * 256 + threadIdx.x" in si
    assert "sil_project_bwd_kernel, dim3(B), dim3(256)" in si and "for (int v = tid; v < V; v += 256)" in si and K["PROJ_BLOCK"] == 256


# ---------------------------------------------------------------------------------------------- collision_ref.py against the oracle
def _pin(verts32, faces):
    tris = verts32.astype(np.float64)[faces]
    want = oc.find_collisions(tris)
    got = cr.find_pairs(verts32, faces)
    assert got.dtype == want.dtype and np.array_equal(got, want), (len(got), len(want))
    assert len(want) > 20
    want_loss = sum(oc.pair_loss(tris[i], tris[j]) for i, j in want)
    loss, per, _ = cr.loss_and_grad(verts32, faces, got)
    assert abs(loss - want_loss) <= 1e-12 * want_loss, (loss, want_loss)
    one = np.array([oc.pair_loss(tris[i], tris[j]) for i, j in want])
    assert np.abs(per - one).max() <= 1e-12 * one.max()
    return got


def test_collision_ref_is_the_oracle():
    v, f = mc.collision_inputs("coll_meshes.spheres")
    for b in range(v.shape[0]):
        pairs = _pin(v[b], f.astype(np.int64))
        assert np.array_equal(pairs, mc.collision_reference("coll_meshes.spheres")[b]["pairs"])
    t, _ = mc.soup(11, 60, 1.0, 0.3)
    _pin(t.reshape(-1, 3), np.arange(180).reshape(60, 3))
    # the gradient of the float64 restatement against central differences of the oracle on one frame's largest entries
    v0, f64 = v[0].astype(np.float64), f.astype(np.int64)
    ref = mc.collision_reference("coll_meshes.spheres")[0]
    for idx in np.argsort(-np.abs(ref["grad"]).ravel())[:6]:
        vi, d = divmod(int(idx), 3)
        vp, vm = v0.copy(), v0.copy()
        vp[vi, d] += 1e-6
        vm[vi, d] -= 1e-6
        fd = (sum(oc.pair_loss(vp[f64][i], vp[f64][j]) for i, j in ref["pairs"]) - sum(oc.pair_loss(vm[f64][i], vm[f64][j]) for i, j in ref["pairs"])) / 2e-6
        assert abs(fd - ref["grad"][vi, d]) <= 1e-6 * np.abs(ref["grad"]).max()


# ---------------------------------------------------------------------------------------------- conditions on the references alone
def test_soups_lose_few_triangles_and_none_grazes():
    for fam in ("coll_tiles", "coll_rounds"):
        for c in mc.CASES[fam]:
            for b, churn in enumerate(mc.soup_churn(c["id"])):
                assert churn <= mc.SOUP_CHURN_CAP * c["F"], (c["id"], b, churn)
            v, f = mc.collision_inputs(c["id"])
            assert f.shape == (c["F"], 3) and v.shape == (c["B"], 3 * c["F"], 3)
            for b in range(c["B"]):
                assert (mc.min_angle(v[b][f]) >= mc.MIN_ANGLE).all()
                _, cand, m = cr.find_pairs(v[b], f, True)
                assert not len(cand) or np.nanmin(np.abs(m)) >= mc.GRAZE, (c["id"], b)


def test_tile_cases_have_the_pairs_they_need():
    for c in mc.CASES["coll_tiles"]:
        ref = mc.collision_reference(c["id"])
        for b, r in enumerate(ref):
            n = len(r["pairs"])
            if c["F"] == 1 or (c["B"] == 3 and b == 1):
                assert n == 0 and r["loss"] == 0.0 and not r["grad"].any(), (c["id"], b)       # the frame between two frames with pairs
            elif c["F"] == 2:
                assert n == 1 and r["loss"] > 0
            else:
                assert n >= c["F"] / 4, (c["id"], b, n)
                assert np.isfinite(r["grad"]).all() and r["e32_grad"].max() > 0
        if c["F"] > mc.CT:           # pairs inside the first tile, inside the second one, and across
            p = ref[0]["pairs"] // mc.CT
            assert {(0, 0), (0, 1)} <= {tuple(x) for x in p} and (c["F"] == mc.CT + 1 or (1, 1) in {tuple(x) for x in p})
    v, f = mc.collision_inputs("coll_tiles.F129.B1")
    assert (cr.candidates(v[0], f)[:, 1] == 128).any()                # the lone triangle of the last tile is somebody's candidate


def test_second_round_case_reaches_every_second_round():
    c = mc.CASES["coll_rounds"][0]
    K = mc.CONSTANTS
    F = c["F"]
    nt = (F + K["CT"] - 1) // K["CT"]
    assert nt == 45 and 5633 <= F <= 5760 and nt * (nt + 1) // 2 == 1035 > K["BROAD_GRID"] > K["TILEPAIR_BLOCK"]
    v, f = mc.collision_inputs(c["id"])
    t = v[0][f]
    lo = np.stack([t[k * K["CT"]:(k + 1) * K["CT"]].min((0, 1)) for k in range(nt)])
    hi = np.stack([t[k * K["CT"]:(k + 1) * K["CT"]].max((0, 1)) for k in range(nt)])
    assert ((lo[:, None] <= hi[None]) & (lo[None] <= hi[:, None])).all()                     # all 1035 tile pairs overlap
    ncand, npair = len(cr.candidates(v[0], f)), len(mc.collision_reference(c["id"])[0]["pairs"])
    print("  second-round case: F = %d, %d candidates (cap %d), %d pairs (cap %d)" % (F, ncand, mc.cand_cap(F), npair, mc.pair_cap(F)))
    assert K["NARROW_THREADS"] < ncand < mc.cand_cap(F)
    assert K["LOSS_THREADS"] < npair < mc.pair_cap(F)


def test_seam_zero_area_and_capacity_cases():
    # the seam: equal positions, different indices; the pair set is the welded one
    v, f, nA = mc.two_spheres()
    vs, fs, ring, copies = mc.seam(v, f, nA)
    assert len(ring) >= 8 and np.array_equal(vs[:, ring], vs[:, copies]) and (fs >= v.shape[1]).any()
    used = np.unique(fs)
    assert set(ring) <= set(used) and set(copies) <= set(used)       # both the original and the copy are somebody's corner
    welded, seamed = mc.collision_reference("coll_meshes.spheres"), mc.collision_reference("coll_meshes.spheres_seam")
    for b in range(2):
        assert np.array_equal(welded[b]["pairs"], seamed[b]["pairs"])
        cand = cr.candidates(vs[b], fs)
        t1, t2 = vs[b][fs][cand[:, 0]], vs[b][fs][cand[:, 1]]
        same = (t1[:, :, None, :] == t2[:, None, :, :]).all(-1).any((1, 2))
        assert same.sum() >= 2 * len(ring)                           # candidates only the equal-position filter removes
        hit, _ = cr.sat(t1[same], t2[same])
        assert hit.all()                                             # ... and every one of them would be reported as a pair
    # the triangle without area: exactly zero cross product in fp32, distinct corners, through the interior of soup triangle 0
    v, f = mc.collision_inputs("coll_zero_area.F129")
    z = v[0][f[-1]]
    e0, e1 = z[1] - z[0], z[2] - z[1]
    n = np.float32([e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]])
    assert z.dtype == np.float32 and not n.any() and len({tuple(p) for p in z}) == 3
    cand = cr.candidates(v[0], f)
    assert ((cand[:, 0] == 0) & (cand[:, 1] == len(f) - 1)).any()
    t0 = v[0][f[0]].astype(np.float64)
    hit, margin = cr.sat(t0[None], z.astype(np.float64)[None])
    assert hit[0] and margin[0] < -1e-2                              # no axis separates them: the SAT alone would report the pair
    nrm = np.cross(t0[1] - t0[0], t0[2] - t0[0])
    s0, s2 = (z[0] - t0[0]) @ nrm, (z[2] - t0[0]) @ nrm
    assert s0 * s2 < 0                                               # the segment crosses the triangle's plane, at its centroid
    base = mc.collision_reference("coll_tiles.F129.B1")[0]
    with_z = mc.collision_reference("coll_zero_area.F129")[0]
    assert np.array_equal(base["pairs"], with_z["pairs"]) and not with_z["grad"][-3:].any()
    tris = v[0].astype(np.float64)[f.astype(np.int64)]
    assert np.array_equal(oc.find_collisions(tris), base["pairs"])   # the oracle decides alike
    # capacities: exactly m^2 candidates, all of them pairs, and the counts the kernel must report
    for c in mc.CASES["coll_caps"]:
        m = c["m"]
        v, f = mc.collision_inputs(c["id"])
        F = len(f)
        cand, pairs = cr.candidates(v[0], f), mc.collision_reference(c["id"])[0]["pairs"]
        assert F == 2 * m and len(cand) == m * m == len(pairs) and (pairs[:, 0] < m).all() and (pairs[:, 1] >= m).all()
        kept_c = min(m * m, mc.cand_cap(F))
        assert c["counts"] == [min(kept_c, mc.pair_cap(F)), m * m - kept_c, kept_c - min(kept_c, mc.pair_cap(F))]
        assert v.shape[1] == 3 * F + 3 and f.max() == 3 * F - 1
        per = mc.collision_reference(c["id"])[0]["per"]
        assert (per > 0).all()


def _chunk_cover(t, size):
    """(chunks, B, size, size) bool: the pixels some triangle of the chunk covers (oracle on the chunk alone)"""
    L = t.shape[1]
    return np.stack([osil.rasterize_fwd(t[:, k:k + mc.CHUNK], size)[0] >= 0 for k in range(0, L, mc.CHUNK)])


def test_silhouette_lists_meet_their_conditions():
    for c in mc.CASES["sil_fwd"]:
        t, fim, alpha = mc.sil_reference(c["id"])
        L, size, B = c["L"], c["size"], c["B"]
        assert t.shape == (B, L, 3, 3) and fim.shape == (B, size, size)
        assert 0.05 < alpha.mean() < 0.95, (c["id"], alpha.mean())
        if L > 1:
            back = (t[..., 2, 1] - t[..., 0, 1]) * (t[..., 1, 0] - t[..., 0, 0]) < (t[..., 1, 1] - t[..., 0, 1]) * (t[..., 2, 0] - t[..., 0, 0])
            assert 0.3 < back.mean() < 0.7                            # both windings
        nch = (L + mc.CHUNK - 1) // mc.CHUNK
        win = np.where(fim >= 0, fim // mc.CHUNK, -1)
        for b in range(B):
            assert all((win[b] == k).any() for k in range(nch)), (c["id"], b)      # every chunk owns winning pixels
        if nch > 1:
            cov = _chunk_cover(t, size)
            multi = cov.sum(0) >= 2
            first = cov.argmax(0)
            last = nch - 1 - cov[::-1].argmax(0)
            later, earlier = int((multi & (win > first)).sum()), int((multi & (win < last)).sum())
            print("  %s: %d pixels where a later chunk wins, %d where an earlier one does" % (c["id"], later, earlier))
            assert later >= 20 and earlier >= 20, (c["id"], later, earlier)
        if L > mc.REPEAT_AT:
            assert np.array_equal(t[:, mc.REPEAT_AT], t[:, mc.REPEAT_SRC])
            without = osil.rasterize_fwd(np.delete(t, mc.REPEAT_SRC, 1), size)[0]
            for b in range(B):
                assert (fim[b] == mc.REPEAT_SRC).any() and not (fim[b] == mc.REPEAT_AT).any()
                assert (without[b] == mc.REPEAT_AT - 1).any()
    for c in mc.CASES["sil_bwd"]:
        t, fim, alpha, g, ref = mc.sil_bwd_reference(c["id"])
        assert np.abs(ref).max() > 0 and not ref[..., 2].any() and (ref != 0).any((2, 3)).sum() >= 50
