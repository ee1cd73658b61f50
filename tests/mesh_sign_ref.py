"""The yardstick of the signed mesh-distance tests: the generalized winding number of a triangle mesh about a point
(Jacobson, Kavan, Sorkine-Hornung 2013), restated with numpy in float64 or, to measure what float32 arithmetic costs, in
float32.

Contract: w(p) = sum over all triangles of Omega / (4 pi), Omega the signed solid angle of van Oosterom & Strackee (1983),
    Omega = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|),   a, b, c = the triangle's corners minus p,
+1 inside a closed mesh whose faces are oriented outward.  A triangle whose edge vectors b - a, c - a are exactly parallel
(repeated index, zero area) contributes exactly 0: its determinant is set to 0, and atan2(0, x >= 0) = 0.  A point on a corner
has a, b or c = 0: determinant and denominator are 0 and atan2(0, 0) = 0.

    winding(P, V, F, dtype)      float64: a plain sum.  float32: every operation in float32 and the triangles added one after
                                 the other in face order (np.add.accumulate), so the rounding of the sum grows like a kernel's
    oriented_box(lo, hi, n)      mesh_dist_ref.box_mesh with every face turned outward (the lo and hi sides of box_mesh share one
                                 index order: half of its faces point inward and its winding numbers are no integers) and one
                                 vertex per position
    hemisphere(...)              the faces of an icosphere whose centroid lies above the centre: an open mesh
    is_closed_ref(F)             every edge used exactly twice, once in each direction (a dictionary, face by face)
"""
import numpy as np

import mesh_dist_ref
from meshes import icosphere


def _dot(x, y):
    return (x * y).sum(-1)


def half_angles(P, V, F, dtype=np.float64):
    """(N, F) atan2 terms: half the signed solid angle of every triangle about every point, all arithmetic in `dtype`"""
    P, V, F = np.asarray(P, dtype), np.asarray(V, dtype), np.asarray(F)
    A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n64 = np.cross(B.astype(np.float64) - A.astype(np.float64), C.astype(np.float64) - A.astype(np.float64))
    area = (n64 != 0).any(1).astype(dtype)                 # 0 for a triangle whose edges are exactly parallel
    a, b, c = A[None] - P[:, None], B[None] - P[:, None], C[None] - P[:, None]
    det = _dot(a, np.cross(b, c)) * area[None]
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(a, c) * lb + _dot(b, c) * la
    h = np.arctan2(det, den)
    assert h.dtype == dtype
    return h


def winding(P, V, F, dtype=np.float64, chunk=256):
    """(N,) generalized winding number of the mesh about every point, as `dtype`"""
    P = np.asarray(P)
    out = np.empty(len(P), dtype)
    for s in range(0, len(P), chunk):
        h = half_angles(P[s:s + chunk], V, F, dtype)
        if dtype == np.float64:
            tot = h.sum(1)
        else:
            tot = np.add.accumulate(h, axis=1, dtype=dtype)[:, -1]
        out[s:s + chunk] = tot * dtype(1.0 / (2.0 * np.pi))
    return out


def oriented_box(lo, hi, n):
    """box_mesh(lo, hi, n) with every face turned so that its normal points away from the box's centre"""
    V, F = mesh_dist_ref.box_mesh(lo, hi, n)
    t = V[F]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    out = _dot(nrm, t.mean(1) - 0.5 * (np.asarray(lo, np.float64) + np.asarray(hi, np.float64)))
    assert (out != 0).all()
    F = np.where((out > 0)[:, None], F, F[:, ::-1])
    # box_mesh gives every side vertices of its own; one vertex per position makes the box a closed mesh by its indices
    _, first, inv = np.unique(np.round(V, 9), axis=0, return_index=True, return_inverse=True)
    return V[first], inv.reshape(-1)[F]


def hemisphere(subdiv=2, radius=1.0, center=(0.0, 0.0, 0.0)):
    """the faces of icosphere(subdiv, radius, center) whose centroid lies above (z) the centre, all of its vertices"""
    V, F = icosphere(subdiv, radius, center)
    unit, _ = icosphere(subdiv)                    # decided on the unit sphere: a centroid on the equator is 0 +- rounding there
    return V, F[unit[F].mean(1)[:, 2] > 1e-9]


def is_closed_ref(F):
    """True when every undirected edge is used by exactly two faces, in opposite directions"""
    seen = {}
    for f in np.asarray(F).tolist():
        for i, j in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if i == j or (i, j) in seen:
                return False
            seen[(i, j)] = True
    return all((j, i) in seen for (i, j) in seen)
