"""GPU: the two mesh terms of the fit -- csrc/collision.hip (chore_collision_fwd / _bwd) and csrc/silhouette.hip (chore_silhouette_fwd /
_bwd, chore_sil_project_fwd / _bwd) -- called directly through the C API at every case of tests/mesh_term_cases.py and compared with
float64: tests/collision_ref.py (pinned to oracle/collision.py on the CPU), oracle/silhouette.py, and the placement / projection
chain as torch expressions.  Outputs live between sentinel margins and are pre-filled with NaN; workspaces have exactly the size
their *_bytes function states, plus a sentinel page (tests/gpu_guards.py).

Bounds.  Collision gradient, per coordinate: |got - ref64| <= 8 E32 + n 2^-25, E32 = the largest |float32 - float64| of the
restatement over the frame's gradient, n = the reference pairs that touch the vertex (one fixed-point rounding each, FX_GRAD = 2^24).
Collision loss: 8 E32_loss + pairs 2^-33.  The pair counts are exact.  Projection: triangles and the three gradients within 8 E32
of the float64 expressions, E32 from the same expressions in float32 on the CPU.  Rasteriser forward: face index and alpha equal
the oracle, every pixel; backward: 1e-4 of the largest entry (the bound of test_gpu_silhouette.py), depth components exactly 0.
Bit for bit: a second run, a permuted face list, a welded against a seamed mesh (loss and counts), a soup with and without a
triangle of zero area.  Every test prints its worst error / E32 ratio; DESIGN.md "Mesh terms: what is checked" records them."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_term_cases as mc
from gpu_guards import Guarded, Workspace, _close
from oracle import silhouette as osil

pytestmark = pytest.mark.gpu

FACTOR = 8.0
RATIO = {}          # family -> worst measured error / E32 of this session


def _env():
    from chore_amd import _lib
    dev = torch.device("cuda", 0)
    return _lib, _lib.lib, _lib.handle(0), dev, torch.cuda.current_stream(dev).cuda_stream


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # a copy: the cases' arrays are read-only


def _raw(g, what):
    """the payload of a Guarded output with its own dtype (the margins checked)"""
    g.read(what)
    return g.buf[g.m:g.m + g.n].cpu().numpy()


def _ratio(family, err, e32, what):
    r = float(err / e32) if e32 > 0 else (0.0 if err == 0 else float("inf"))
    if r > RATIO.get(family, -1.0):
        RATIO[family] = r
        print("  worst so far %-12s error / E32 = %.3f   at %s" % (family, r, what))
    return r


# ================================================================================================ chore_collision_fwd / _bwd
def _collide(verts, faces, with_counts=True):
    """-> loss (B,) float32, gverts (B,V,3) float32, counts (B + 2,) int32 or None; the guards and the workspace page checked"""
    _lib, L, h, dev, stream = _env()
    B, V, _ = verts.shape
    F = faces.shape[0]
    v, f = _dev(verts, dev), _dev(faces, dev)
    nbytes = L.chore_collision_workspace_bytes(B, V, F)
    ws = Workspace(nbytes, dev)
    loss, grad = Guarded(B, dev), Guarded(B * V * 3, dev)
    counts = Guarded(B + 2, dev, dtype=torch.int32, fill=-1) if with_counts else None
    _lib.check(L.chore_collision_fwd(h, v.data_ptr(), f.data_ptr(), B, V, F, loss.ptr, grad.ptr, counts.ptr if counts else None, ws.ptr,
                                     stream), h, "chore_collision_fwd")
    torch.cuda.synchronize()
    ws.check("chore_collision_fwd")
    return (_raw(loss, "collision loss"), _raw(grad, "collision gradient").reshape(B, V, 3),
            _raw(counts, "collision counts") if counts else None)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %d entries differ" % (what, int((a != b).sum()))


def _check_against_reference(cid, loss, grad, counts, family):
    ref = mc.collision_reference(cid)
    assert np.isfinite(loss).all() and np.isfinite(grad).all(), cid
    assert counts.tolist() == [len(r["pairs"]) for r in ref] + [0, 0], (cid, counts.tolist(), [len(r["pairs"]) for r in ref])
    for b, r in enumerate(ref):
        what = "%s frame %d" % (cid, b)
        if not len(r["pairs"]):
            assert loss[b] == 0.0 and not grad[b].any(), "%s: a frame without pairs must come out exactly zero" % what
            continue
        err = abs(float(loss[b]) - r["loss"])
        _ratio(family + " loss", err, r["e32_loss"], what)
        bound = FACTOR * r["e32_loss"] + len(r["pairs"]) * 2.0 ** -33
        assert err <= bound, "%s: loss %.9g, reference %.9g, error %.3e, bound %.3e" % (what, loss[b], r["loss"], err, bound)
        e32 = float(r["e32_grad"].max())
        d = np.abs(grad[b].astype(np.float64) - r["grad"])
        _ratio(family + " grad", d.max(), e32, what)
        bound = FACTOR * e32 + r["n"][:, None] * 2.0 ** -25
        bad = d > bound
        assert not bad.any(), "%s: %d gradient coordinates beyond 8 E32 + n 2^-25 (E32 %.3e), worst %.3e at %s" % (
            what, int(bad.sum()), e32, d.max(), np.unravel_index(d.argmax(), d.shape))
        assert not grad[b][r["n"] == 0].any(), "%s: a vertex of no colliding triangle has a gradient" % what


def _run_and_check(cid, family):
    verts, faces = mc.collision_inputs(cid)
    loss, grad, counts = _collide(verts, faces)
    _check_against_reference(cid, loss, grad, counts, family)
    again = _collide(verts, faces, with_counts=False)                   # counts = NULL, as the fit calls it
    _same_bits(loss, again[0], cid + " loss, second run")
    _same_bits(grad, again[1], cid + " gradient, second run")
    return verts, faces, loss, grad, counts


@pytest.mark.parametrize("case", mc.CASES["coll_tiles"], ids=mc.ids("coll_tiles"))
def test_collision_tile_edges(case):
    """F one below, equal to and one above a tile and two tiles; a frame without pairs between two frames with pairs; _bwd"""
    verts, faces, loss, grad, counts = _run_and_check(case["id"], "coll_tiles")
    _lib, L, h, dev, stream = _env()
    B, V, _ = verts.shape
    gout = np.random.RandomState(case["F"] + case["B"]).standard_normal(B).astype(np.float32)
    out = Guarded(B * V * 3, dev)
    gv, go = _dev(grad, dev), _dev(gout, dev)
    _lib.check(L.chore_collision_bwd(h, gv.data_ptr(), go.data_ptr(), B, V, out.ptr, stream), h, "chore_collision_bwd")
    torch.cuda.synchronize()
    _same_bits(_raw(out, "collision bwd").reshape(B, V, 3) + np.float32(0), gout[:, None, None] * grad + np.float32(0), case["id"] + " bwd")


@pytest.mark.parametrize("case", mc.CASES["coll_rounds"], ids=mc.ids("coll_rounds"))
def test_collision_second_rounds(case):
    """45 tiles: 1035 tile pairs for 1024 workgroups, more candidates and pairs than the narrow and loss grids have threads"""
    _run_and_check(case["id"], "coll_rounds")


@pytest.mark.parametrize("case", mc.CASES["coll_meshes"], ids=mc.ids("coll_meshes"))
def test_collision_meshes(case):
    """two icospheres, full gradient; the same with a ring of duplicated vertices: loss and counts equal the welded run bit for bit,
    a ring vertex' gradient and its copy's sum to the welded vertex' gradient"""
    cid = case["id"]
    if case["kind"] == "spheres":
        _run_and_check(cid, "coll_meshes")
        return
    verts, faces = mc.collision_inputs(cid)
    loss, grad, counts = _collide(verts, faces)
    w_verts, w_faces, nA = mc.two_spheres()
    _, _, ring, copies = mc.seam(w_verts, w_faces, nA)
    w_loss, w_grad, w_counts = _collide(w_verts, w_faces)
    _same_bits(loss, w_loss, cid + " loss against the welded mesh")
    _same_bits(counts, w_counts, cid + " counts against the welded mesh")
    V = w_verts.shape[1]
    folded = grad[:, :V].astype(np.float64)
    folded[:, ring] += grad[:, copies].astype(np.float64)
    assert np.abs(grad[:, copies]).max() > 0 and np.abs(grad[:, ring]).max() > 0
    for b, r in enumerate(mc.collision_reference("coll_meshes.spheres")):
        e32 = float(r["e32_grad"].max())
        d = np.abs(folded[b] - r["grad"])
        _ratio("coll_meshes grad", d.max(), e32, "%s frame %d" % (cid, b))
        assert not (d > FACTOR * e32 + r["n"][:, None] * 2.0 ** -25).any(), (cid, b, d.max(), e32)
    keep = np.setdiff1d(np.arange(V), ring)
    _same_bits(np.ascontiguousarray(grad[:, keep]), np.ascontiguousarray(w_grad[:, keep]), cid + " gradient off the seam")


@pytest.mark.parametrize("case", mc.CASES["coll_order"], ids=mc.ids("coll_order"))
def test_collision_order_independence(case):
    """a seeded permutation of the faces fills every list in another order: losses, counts and all gradients bit for bit"""
    v0, f0 = mc.collision_inputs(case["of"])
    v1, f1 = mc.collision_inputs(case["id"])
    assert np.array_equal(v0, v1) and not np.array_equal(f0, f1) and np.array_equal(np.sort(f0.view("i4,i4,i4"), 0), np.sort(f1.view("i4,i4,i4"), 0))
    a, b = _collide(v0, f0), _collide(v1, f1)
    for x, y, name in zip(a, b, ("loss", "gradient", "counts")):
        _same_bits(x, y, "%s %s under a permutation of the faces" % (case["id"], name))


@pytest.mark.parametrize("case", mc.CASES["coll_zero_area"], ids=mc.ids("coll_zero_area"))
def test_collision_zero_area_triangle(case):
    """a triangle without area that pierces a soup triangle forms no pair: everything finite, counts, loss and all other gradients
    as without it, bit for bit; its own gradient exactly zero"""
    v0, f0 = mc.collision_inputs(case["of"])
    v1, f1 = mc.collision_inputs(case["id"])
    base, got = _collide(v0, f0), _collide(v1, f1)
    print("  %s: loss %r (without the triangle %r), counts %s (%s), gradient of the triangle %s, non-finite gradient entries %d" % (
        case["id"], got[0].tolist(), base[0].tolist(), got[2].tolist(), base[2].tolist(), got[1][0, -3:].tolist(), int((~np.isfinite(got[1])).sum())))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), "non-finite output"
    _same_bits(got[2], base[2], case["id"] + " counts")
    _same_bits(got[0], base[0], case["id"] + " loss")
    _same_bits(np.ascontiguousarray(got[1][:, :-3]), base[1], case["id"] + " gradients of the soup")
    assert not got[1][:, -3:].any(), "the triangle without area has a gradient"
    _check_against_reference(case["id"], *got, "coll_zero")


@pytest.mark.parametrize("case", mc.CASES["coll_caps"], ids=mc.ids("coll_caps"))
def test_collision_full_lists(case):
    """more pairs (m = 64) and more candidates (m = 100) than the lists hold: the written behaviour -- nothing is written past a
    list, the counts say what was kept and what was dropped, the result is a finite sum over pair_cap of the pairs"""
    verts, faces = mc.collision_inputs(case["id"])
    loss, grad, counts = _collide(verts, faces)                         # checks the sentinel page behind the exact-size workspace
    assert counts.tolist() == case["counts"], (counts.tolist(), case["counts"])
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    r = mc.collision_reference(case["id"])[0]
    per, cap = np.sort(r["per"]), mc.pair_cap(len(faces))
    lo, hi = per[:cap].sum(), per[-cap:].sum()
    print("  %s: loss %.6g between %.6g and %.6g (all %d pairs: %.6g)" % (case["id"], loss[0], lo, hi, len(per), per.sum()))
    assert lo <= float(loss[0]) <= hi
    assert (r["n"] == 0).sum() == 3 and not grad[0][r["n"] == 0].any() and np.abs(grad[0]).max() > 0


# ================================================================================================ chore_silhouette_fwd / _bwd
def _rasterize(t, size):
    _lib, L, h, dev, stream = _env()
    B, Fn = t.shape[:2]
    tri = _dev(t, dev)
    nbytes = L.chore_silhouette_workspace_bytes(B, Fn)
    ws = Workspace(nbytes, dev)
    fim, alpha = Guarded(B * size * size, dev, dtype=torch.int32, fill=-7), Guarded(B * size * size, dev)
    _lib.check(L.chore_silhouette_fwd(h, tri.data_ptr(), B, Fn, size, float(osil.NEAR), float(osil.FAR), fim.ptr, alpha.ptr, ws.ptr, stream),
               h, "chore_silhouette_fwd")
    torch.cuda.synchronize()
    ws.check("chore_silhouette_fwd")
    return _raw(fim, "face_index").reshape(B, size, size), _raw(alpha, "alpha").reshape(B, size, size)


@pytest.mark.parametrize("case", mc.CASES["sil_fwd"], ids=mc.ids("sil_fwd"))
def test_silhouette_forward(case):
    """lists of one below, equal to, one above and more than two chunks at sizes that are no multiple of the tile: the winner of
    every pixel (carried across chunks, ties to the smaller index) and alpha equal the oracle"""
    t, fim_o, alpha_o = mc.sil_reference(case["id"])
    fim, alpha = _rasterize(t, case["size"])
    ne = fim != fim_o
    assert not ne.any(), "%s: %d pixels with another winner, first at %s: %d instead of %d" % (
        case["id"], int(ne.sum()), tuple(np.argwhere(ne)[0]), fim[tuple(np.argwhere(ne)[0])], fim_o[tuple(np.argwhere(ne)[0])])
    _same_bits(alpha, alpha_o, case["id"] + " alpha")


@pytest.mark.parametrize("case", mc.CASES["sil_bwd"], ids=mc.ids("sil_bwd"))
def test_silhouette_backward(case):
    t, fim_o, alpha_o, g, ref = mc.sil_bwd_reference(case["id"])
    fim, alpha = _rasterize(t, case["size"])
    assert np.array_equal(fim, fim_o)
    _lib, L, h, dev, stream = _env()
    B, Fn = t.shape[:2]
    out = Guarded(B * Fn * 9, dev)
    bufs = [_dev(a, dev) for a in (t, fim, alpha, g)]
    _lib.check(L.chore_silhouette_bwd(h, *[x.data_ptr() for x in bufs], B, Fn, case["size"], float(osil.EPS), out.ptr, stream), h,
               "chore_silhouette_bwd")
    torch.cuda.synchronize()
    got = out.read("grad_faces").reshape(B, Fn, 3, 3)
    _close(got, ref.astype(np.float64), "sil_bwd " + case["id"], 1e-4)
    assert not got[..., 2].any(), "silhouettes carry no depth gradient"
    assert not got[~(ref != 0).any((2, 3))].any()


# ================================================================================================ chore_sil_project_fwd / _bwd
@pytest.mark.parametrize("case", mc.CASES["sil_project"], ids=mc.ids("sil_project"))
def test_silhouette_projection(case):
    """placement, projection with and without distortion, both windings, and the pull-back to dRo, dto, ds: V and 2F one below,
    equal to and one above a block of 256 and several blocks, one camera for all frames and one per frame, orig_size 1 and 2"""
    _lib, L, h, dev, stream = _env()
    d = mc.project_inputs(case["id"])
    (tri_r, dR_r, dt_r, ds_r), e32 = mc.project_reference(case["id"])
    B, V, F = case["B"], case["V"], case["F"]
    t = {k: _dev(d[k], dev) for k in ("verts", "faces", "Ro", "to", "s", "K", "cam_R", "cam_t", "g", "adj_off", "adj")}
    dist = None if d["dist5"] is None else (ctypes.c_float * 5)(*[float(x) for x in d["dist5"]])
    tri = Guarded(B * 2 * F * 9, dev)
    _lib.check(L.chore_sil_project_fwd(h, t["verts"].data_ptr(), t["faces"].data_ptr(), t["Ro"].data_ptr(), t["to"].data_ptr(), t["s"].data_ptr(),
                                       t["K"].data_ptr(), t["cam_R"].data_ptr(), t["cam_t"].data_ptr(), case["bcast"], dist, d["orig"], d["eps"],
                                       B, V, F, tri.ptr, stream), h, "chore_sil_project_fwd")
    dR, dt, ds = Guarded(B * 9, dev), Guarded(B * 3, dev), Guarded(B, dev)
    _lib.check(L.chore_sil_project_bwd(h, t["verts"].data_ptr(), t["Ro"].data_ptr(), t["to"].data_ptr(), t["s"].data_ptr(), t["K"].data_ptr(),
                                       t["cam_R"].data_ptr(), t["cam_t"].data_ptr(), case["bcast"], dist, d["orig"], d["eps"], B, V, F,
                                       t["adj_off"].data_ptr(), t["adj"].data_ptr(), t["g"].data_ptr(), dR.ptr, dt.ptr, ds.ptr, stream), h,
               "chore_sil_project_bwd")
    torch.cuda.synchronize()
    for got, ref, e, name in ((tri.read("tri").reshape(tri_r.shape), tri_r, e32[0], "tri"), (dR.read("dRo").reshape(dR_r.shape), dR_r, e32[1], "dRo"),
                              (dt.read("dto").reshape(dt_r.shape), dt_r, e32[2], "dto"), (ds.read("ds").reshape(ds_r.shape), ds_r, e32[3], "ds")):
        assert np.isfinite(got).all(), (case["id"], name)
        err = float(np.abs(got - ref).max())
        _ratio("sil_project " + name, err, e, case["id"])
        assert err <= FACTOR * e, "%s %s: error %.3e, E32 %.3e (ratio %.2f, bound 8), largest entry %.3g" % (case["id"], name, err, e, err / e, np.abs(ref).max())
