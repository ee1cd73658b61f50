"""CPU: the float64 restatement of the ordinal depth term (tests/ordinal_depth_ref.py) against torch float64 autograd of the
composed expression (clamp, softplus, masks), on a box scene and on the fixture's 40-vertex template, with pixels whose two
depths are exactly equal and pixels whose difference exceeds the clamp; and its float32 error bounds against a float32
evaluation of the depth rule on the host."""
import functools

import numpy as np
import pytest
import torch

import ordinal_depth_ref as odr
import render_bwd_ref
import render_ref
from conftest import golden

FOCAL = 6.0
S = 40          # partial 16 x 16 tiles, 1 600 pixels: no multiple of a 256-pixel block


def _object(kind):
    if kind == "box":
        return odr.box_verts(), odr.BOX_FACES
    g = golden("sil_project.npz")
    v = g["verts"].astype(np.float64)
    return ((v - v.mean(0)) * 0.8).astype(np.float32), g["faces"].astype(np.int64)


def _body():
    """a stand-in occluder: two large tilted quads (four triangles) across the view at depths 2.9 .. 3.3"""
    v = np.array([[-1.2, -1.3, 2.9], [0.1, -1.3, 3.2], [0.1, 1.3, 3.3], [-1.2, 1.3, 3.0],
                  [0.0, -1.3, 3.25], [1.2, -1.3, 2.95], [1.2, 1.3, 3.05], [0.0, 1.3, 3.3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int64)
    return v, f


@functools.lru_cache(maxsize=None)
def scene(kind):
    """B = 2 frames.  Frame 0: the object straddles the body's surface (both cases occur) and the object's two faces that win most
    pixels are part of the occluder as well (exactly equal depths there); frame 1: the body about 2.8 behind the object in the
    left half and about 2.8 in front of it in the right half (differences beyond c = 2, both cases)."""
    ov, of = _object(kind)
    bv, bf = _body()
    R = odr.rot_xyz(0.5, 0.4, 0.2)
    placed = [ov @ R.T + np.array([0.05, -0.05, 3.3], np.float32), None]
    placed[1] = ov + np.array([0.0, 0.0, 3.1], np.float32)
    tri = np.stack([odr.pinhole_tri(p.astype(np.float32), of, FOCAL) for p in placed])
    fim = render_ref.winners(tri, S)
    ids, n = np.unique(fim[0][fim[0] >= 0] % len(of), return_counts=True)
    shared = ids[np.argsort(-n)[:2]]
    occ_tri, occ_same = [], []
    for b in range(2):
        v = np.concatenate([bv, placed[b].astype(np.float32)])
        f = np.concatenate([bf, of[shared] + len(bv)]) if b == 0 else bf
        occ_tri.append(odr.pinhole_tri(v, f, FOCAL))
        occ_same.append(len(bf) if b == 0 else None)
    same = np.zeros((2, S, S), bool)
    occ = np.empty((2, S, S), np.float32)
    for b in range(2):
        t = occ_tri[b][None]
        w = render_ref.winners(t, S)
        occ[b] = odr_depth32(t, 0, w)[::-1]           # float32, image_ref's orientation: an input of the kernel
        if occ_same[b] is not None:
            nb, nf = occ_same[b], len(occ_tri[b]) // 2
            for j, face in enumerate(shared):          # occluder face nb + j (either winding) is object face `face` (same winding)
                for wind in (0, 1):
                    same[b] |= ((w[0] == nb + j + wind * nf) & (fim[b] == face + wind * len(of)))[::-1]
    # frame 1: the body 2.8 behind the object in the left half, 2.8 in front of it in the right half
    occ[1, :, : S // 2] = np.where(occ[1, :, : S // 2] < 100, occ[1, :, : S // 2] + np.float32(2.8), occ[1, :, : S // 2])
    occ[1, :, S // 2:] = np.where(occ[1, :, S // 2:] < 100, occ[1, :, S // 2:] - np.float32(2.8), occ[1, :, S // 2:])
    image_ref, keep = odr.block_masks(2, S, 5)
    return dict(tri=tri, fim=fim, occ=occ, same=same, image_ref=image_ref, keep=keep)


@pytest.mark.parametrize("kind", ["box", "template"])
def test_restatement_against_autograd(kind):
    c = scene(kind)
    ref = odr.forward(c["tri"], c["fim"], c["occ"], c["image_ref"], c["keep"], same=c["same"])
    print("%s: counts %s, ties %d, beyond c %d, depth bound: median %.3e, largest %.3e" %
          (kind, ref["counts"].tolist(), int(ref["tie"].sum()), int(ref["beyond"].sum()),
           float(np.median(ref["d_err"][ref["d_err"] > 0])), float(ref["d_err"].max())))
    assert ref["tie"].sum() > 0 and ref["beyond"].sum() > 0
    assert (ref["counts"][:, :2].sum(0) > 0).all() and ((ref["case_a"] | ref["case_b"]) & ~ref["beyond"])[0].any()
    assert (ref["case_a"] & ref["case_b"]).sum() == 0 and not (ref["tie"] & (ref["case_a"] | ref["case_b"])).any()
    # the composed expression in torch float64, differentiated by autograd with respect to the object's depth image
    dh = torch.tensor(c["occ"].astype(np.float64))
    d0 = np.where(c["same"], c["occ"].astype(np.float64), ref["d_o"])
    d = torch.tensor(d0, requires_grad=True)
    O = torch.tensor(c["image_ref"] > 0.5)
    P = ~O & torch.tensor(c["keep"] < 0.5)
    both = torch.tensor(c["fim"][:, ::-1].copy() >= 0) & (dh < 100.0)
    a = P & both & (d < dh)
    b = O & both & (dh < d)
    sp = torch.nn.functional.softplus
    terms = a * sp(torch.clamp(dh - d, max=odr.C)) + b * sp(torch.clamp(d - dh, max=odr.C))
    terms.sum().backward()
    counts = torch.stack([a.sum((1, 2)), b.sum((1, 2)), (P & both).sum((1, 2)), (O & both).sum((1, 2))], 1)
    assert np.array_equal(counts.numpy(), ref["counts"])
    assert np.abs(terms.detach().numpy() - ref["terms"]).max() <= 1e-13
    assert np.abs(d.grad.numpy() - ref["coef"]).max() <= 1e-13
    assert (ref["coef"][ref["beyond"]] == 0).all() and (ref["terms"][ref["beyond"]] == np.log1p(np.exp(odr.C))).all()
    assert (ref["coef"][ref["tie"]] == 0).all() and (ref["terms"][ref["tie"]] == 0).all()
    assert np.array_equal(ref["sums"], ref["terms"].sum((1, 2)))


def odr_depth32(tri, b, fim):
    """(S,S) float32 depth image of frame b (rows of the winner map) by the depth rule in float32, FAR where nothing won"""
    yi, xi, _, _, zp, _, _ = render_bwd_ref._winner_terms(np.asarray(tri, np.float32), b, fim, np.float32)
    d = np.full(fim.shape[1:], np.float32(odr.FAR), np.float32)
    d[yi, xi] = zp
    return d


@pytest.mark.parametrize("kind", ["box", "template"])
def test_error_bounds_hold_for_a_float32_evaluation(kind):
    """the depth rule evaluated in float32 on the host (tests/render_bwd_ref.py, the kernel's operation order) stays within the
    running bound at every winner pixel; the backward restatement runs, agrees with render_bwd_ref.depth_bwd (asserted inside)
    and bounds a float32 evaluation of the same sums"""
    c = scene(kind)
    worst = 0.0
    for b in range(2):
        yi, xi, fn, w, zp, inv, z = odr.depth_rule(c["tri"], b, c["fim"])
        z32 = render_bwd_ref._winner_terms(c["tri"].astype(np.float32), b, c["fim"], np.float32)[4]
        err = np.abs(z32.astype(np.float64) - zp.v)
        assert (err <= zp.e).all()
        worst = max(worst, float((err / zp.e).max()))
    print("%s: float32 depth, largest |error| / bound %.3f" % (kind, worst))
    d32 = np.stack([odr_depth32(c["tri"], b, c["fim"]) for b in range(2)])[:, ::-1]
    ref = odr.forward(c["tri"], c["fim"], c["occ"], c["image_ref"], c["keep"], d32=d32)
    pure = odr.forward(c["tri"], c["fim"], c["occ"], c["image_ref"], c["keep"], same=c["same"])
    print("%s: decisions on the float32 depths: counts %s, ties %d (by construction %d), depth ratio %.3f"
          % (kind, ref["counts"].tolist(), int(ref["tie"].sum()), int(pure["tie"].sum()), ref["depth_ratio"]))
    assert ref["depth_ratio"] <= 1 and np.array_equal(ref["tie"], pure["tie"])         # the shared triangles tie in float32 too
    assert np.abs(ref["counts"] - pure["counts"]).max() <= 3                           # (a float64 depth within round-off of d_h)
    g = np.array([1.5, -0.5], np.float32)
    coef32 = ref["coef"].astype(np.float32)
    val, err = odr.backward(c["tri"], c["fim"], coef32, g)
    got32 = render_bwd_ref.depth_bwd(c["tri"], c["fim"], (coef32 * g[:, None, None])[:, ::-1], np.float32)
    assert np.isfinite(val).all() and np.abs(val).max() > 0
    d = np.abs(got32.astype(np.float64) - val)
    print("%s: float32 backward, largest |error| / bound %.3f" % (kind, float((d / np.maximum(err, 1e-300)).max())))
    assert (d <= err).all()
    assert (val[0] != 0).any() and not val[1].any()          # frame 1: every difference exceeds c, no gradient at all
