"""Vectorised float64 restatement of oracle/collision.py for the cases of tests/mesh_term_cases.py (no GPU needed).

The oracle walks the triangles in Python loops: fine at 800 faces, hopeless at the 5 700 of the second-round case.  Here the same
steps are array expressions, and each returns what the tests need besides the decision:
  candidates(verts32, faces)      pairs i < j whose float32 boxes overlap and that share no vertex INDEX (what coll_broad_kernel lists)
  sat(t1, t2)                     the 17-axis separating-axis test: decision (the oracle's comparisons on the unnormalised axes) and
                                  margin = the largest separating gap (positive) or minus the smallest overlap over the axes
                                  (negative), along the unit axis, in units of the longest edge of the two triangles
  find_pairs(verts32, faces)      candidates without equal POSITIONS (the narrow phase's `same`), without a triangle of zero area (a
                                  triangle without area has no cone and no interior: it forms no pair) and not separated
  pair_losses(t1, t2)             torch, any dtype: the two cone fields of every pair
  loss_and_grad(verts, faces, pairs, dtype)   sum over the FIXED pair set and its gradient w.r.t. all vertices by autograd
tests/test_mesh_term_coverage_table.py pins pairs and losses to oracle/collision.py."""
import numpy as np
import torch

SIGMA = 0.5


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def candidates(verts32, faces, rows=512):
    """(V,3) float32, (F,3) int -> (C,2) int64, i < j, lexicographic: boxes overlap (<=, on the float32 coordinates), no shared index"""
    verts32, faces = np.asarray(verts32), np.asarray(faces, np.int64)
    assert verts32.dtype == np.float32
    tris = verts32[faces]
    lo, hi = tris.min(1), tris.max(1)
    n = len(faces)
    out = []
    for r0 in range(0, n, rows):
        r1 = min(r0 + rows, n)
        ov = ((lo[r0:r1, None] <= hi[None]) & (lo[None] <= hi[r0:r1, None])).all(-1)
        ov &= np.arange(n)[None] > np.arange(r0, r1)[:, None]
        i, j = np.nonzero(ov)
        i += r0
        share = (faces[i][:, :, None] == faces[j][:, None, :]).any((1, 2))
        out.append(np.stack([i[~share], j[~share]], 1))
    return np.concatenate(out, 0).astype(np.int64).reshape(-1, 2)


def sat(t1, t2):
    """(C,3,3), (C,3,3) float64 -> (intersect (C,) bool, margin (C,) float64).  An axis of zero length separates nothing."""
    t1, t2 = np.asarray(t1, np.float64), np.asarray(t2, np.float64)
    e1 = np.stack([t1[:, 1] - t1[:, 0], t1[:, 2] - t1[:, 1], t1[:, 0] - t1[:, 2]], 1)
    e2 = np.stack([t2[:, 1] - t2[:, 0], t2[:, 2] - t2[:, 1], t2[:, 0] - t2[:, 2]], 1)
    n1, n2 = _cross(e1[:, 0], e1[:, 1]), _cross(e2[:, 0], e2[:, 1])
    axes = [n1, n2] + [_cross(e1[:, p], e2[:, q]) for p in range(3) for q in range(3)]
    axes += [_cross(n1, e1[:, p]) for p in range(3)] + [_cross(n2, e2[:, p]) for p in range(3)]
    ax = np.stack(axes, 1)                                          # (C,17,3)
    p1, p2 = np.einsum("ckd,cad->cak", t1, ax), np.einsum("ckd,cad->cak", t2, ax)
    gap = np.maximum(p2.min(-1) - p1.max(-1), p1.min(-1) - p2.max(-1))        # > 0: the axis separates
    intersect = ~(gap > 0).any(-1)
    norm = np.sqrt((ax * ax).sum(-1))
    size = np.sqrt(np.maximum((e1 * e1).sum(-1).max(-1), (e2 * e2).sum(-1).max(-1)))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(norm > 0, gap / (norm * size[:, None]), -np.inf)
    sep = rel.max(-1)
    overlap = np.where(norm > 0, -rel, np.inf).min(-1)
    return intersect, np.where(intersect, -overlap, sep)


def areas_zero(tris):
    e0, e1 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 1]
    n = _cross(e0, e1)
    return (n * n).sum(-1) == 0


def find_pairs(verts32, faces, with_margin=False):
    """-> (P,2) int64 pairs (i < j, lexicographic) [, candidates (C,2), their margins (C,) (nan where the narrow phase never asks)]"""
    verts32, faces = np.asarray(verts32), np.asarray(faces, np.int64)
    cand = candidates(verts32, faces)
    tris = verts32[faces].astype(np.float64)
    t1, t2 = tris[cand[:, 0]], tris[cand[:, 1]]
    same = (t1[:, :, None, :] == t2[:, None, :, :]).all(-1).any((1, 2))
    flat = areas_zero(tris)
    ask = ~same & ~flat[cand[:, 0]] & ~flat[cand[:, 1]]
    hit, margin = sat(t1[ask], t2[ask])
    pairs = cand[ask][hit]
    if not with_margin:
        return pairs
    m = np.full(len(cand), np.nan)
    m[ask] = margin
    return pairs, cand, m


def _cone_field(pts, tri, sigma):
    """torch: (P,3,3) points, (P,3,3) cone triangles -> (P,) sum over the three points of Psi^2"""
    a, b = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    c = torch.linalg.cross(a, b)
    aa, bb, cc = (a * a).sum(-1), (b * b).sum(-1), (c * c).sum(-1)
    ab = a - b
    r = torch.sqrt(aa * bb * (ab * ab).sum(-1) / (4 * cc))
    o = tri[:, 0] + torch.linalg.cross(aa[:, None] * b - bb[:, None] * a, c) / (2 * cc)[:, None]
    n = c / torch.sqrt(cc)[:, None]
    d = pts - o[:, None]
    x = (d * n[:, None]).sum(-1)                                    # (P,3)
    q = d - x[..., None] * n[:, None]
    qq = (q * q).sum(-1)
    rad = torch.where(qq > 0, torch.sqrt(torch.where(qq > 0, qq, torch.ones_like(qq))), torch.zeros_like(qq))   # |.| at 0: subgradient 0
    live = x < sigma
    den = torch.where(live, r[:, None] - (r[:, None] * x) / sigma, torch.ones_like(x))
    phi = rad / den
    mid = -(1 - 2 * sigma) / (4 * sigma ** 2) * x * x - x / (2 * sigma) + (3 - 2 * sigma) / 4
    ups = torch.where(x <= -sigma, -x + 1 - sigma, mid)
    psi = torch.where(live & (phi < 1), (1 - phi) * ups, torch.zeros_like(x))
    return (psi * psi).sum(-1)


def pair_losses(t1, t2, sigma=SIGMA):
    """cone of t1 over the points of t2 plus cone of t2 over the points of t1 (oracle.collision.pair_loss), per pair"""
    return _cone_field(t2, t1, sigma) + _cone_field(t1, t2, sigma)


def loss_and_grad(verts32, faces, pairs, dtype=torch.float64):
    """the fixed pair set's loss (float), per-pair losses (P,) and gradient (V,3), computed in `dtype`, returned as float64 numpy"""
    v = torch.tensor(np.asarray(verts32), dtype=dtype, requires_grad=True)
    f = torch.as_tensor(np.asarray(faces, np.int64))
    if len(pairs) == 0:
        return 0.0, np.zeros(0), np.zeros(v.shape, np.float64)
    tris = v[f]
    per = pair_losses(tris[torch.as_tensor(pairs[:, 0])], tris[torch.as_tensor(pairs[:, 1])])
    total = per.sum()
    total.backward()
    return float(total.detach().double()), per.detach().double().numpy(), v.grad.double().numpy()


def touches(faces, pairs, V):
    """(V,) number of pairs that touch each vertex: the count of fixed-point roundings its gradient coordinates may collect"""
    n = np.zeros(V, np.int64)
    faces = np.asarray(faces, np.int64)
    if len(pairs):
        np.add.at(n, faces[pairs.ravel()].ravel(), 1)
    return n
