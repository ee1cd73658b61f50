"""The yardstick of the mesh-distance gradient tests: the gradient of the exact point-to-mesh distance with respect to the
points and the mesh vertices, restated with numpy on top of tests/mesh_dist_ref.py, in float64 or, to measure what float32
arithmetic costs, in float32.

For a point p with winning triangle (a0, a1, a2) (mesh_dist_ref: smallest distance, first triangle attaining it), closest
point c = sum_k b_k a_k and d = |p - c| > 0, n = (p - c) / d:
    dd/dp = n        dd/da_k = -b_k n        (vertex, edge and interior regions alike: d is a minimum over b)
and zero rows where d == 0.  b are the barycentric coordinates of c in its triangle: those of the closest point of p on the
winning triangle by its Voronoi regions, clamped to [0, 1] with b_0 = 1 - b_1 - b_2; a triangle without an area is the
segment or point it degenerates to (the weights of the nearest foot point of p on its three edges).

    grads(P, V, F, g, dtype)       D, I, C, bary, dP (N,3), dV (V,3); dV accumulated in ascending point order, corners 0, 1, 2
    e32_dist(P, V, F)              largest |float32 - float64| of the restated distance
    ties(P, V, F, tol)             points where a triangle with a DIFFERENT closest point (farther than 1e-3 bounding-box
                                   diagonals from the winner's) is within `tol` of the winning distance: the distance is not
                                   differentiable there (medial axis), the tests leave them out
    fd_points / fd_verts           central differences of sum_i g_i d_i in float64
    sphere_pair / descent          the two-sphere interpenetration case and its float64 descent
"""
import numpy as np

import mesh_dist_ref as ref
from meshes import icosphere


def _dot(x, y):
    return (x * y).sum(-1)


def barycentric(q, a, b, c):
    """(N,3) weights of the closest point of q on the triangles (a, b, c), all (N,3) of one float dtype: clamped, summing to 1"""
    dt = q.dtype.type
    zero, one = dt(0), dt(1)
    ab, ac, aq = b - a, c - a, q - a
    aa, cc, e = _dot(ab, ab), _dot(ac, ac), _dot(ab, ac)
    d1, d2 = _dot(ab, aq), _dot(ac, aq)
    det = aa * cc - e * e
    ok = det > dt(1e-12) * aa * cc
    # the Voronoi regions of the triangle (Ericson 5.1.5; mesh_dist_ref._voronoi gives the point, this the weights): a point
    # beyond a corner gives the other two corners exactly 0
    d3, d4 = _dot(ab, q - b), _dot(ac, q - b)
    d5, d6 = _dot(ab, q - c), _dot(ac, q - c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    den = va + vb + vc
    b1, b2 = ref._sdiv(vb, den), ref._sdiv(vc, den)                                       # interior
    w = ref._sdiv(d4 - d3, (d4 - d3) + (d5 - d6))
    m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
    b1, b2 = np.where(m, one - w, b1), np.where(m, w, b2)                                 # edge bc
    m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    b1, b2 = np.where(m, zero, b1), np.where(m, ref._sdiv(d2, d2 - d6), b2)               # edge ac
    m = (d6 >= 0) & (d5 <= d6)
    b1, b2 = np.where(m, zero, b1), np.where(m, one, b2)                                  # corner c
    m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    b1, b2 = np.where(m, ref._sdiv(d1, d1 - d3), b1), np.where(m, zero, b2)               # edge ab
    m = (d3 >= 0) & (d4 <= d3)
    b1, b2 = np.where(m, one, b1), np.where(m, zero, b2)                                  # corner b
    m = (d1 <= 0) & (d2 <= 0)
    b1, b2 = np.where(m, zero, b1), np.where(m, zero, b2)                                 # corner a
    b1 = np.clip(b1, zero, one)
    b2 = np.minimum(np.clip(b2, zero, one), one - b1)

    def foot(o, ev, qq):
        ee = _dot(ev, ev)
        t = np.clip(ref._sdiv(_dot(qq - o, ev), ee), dt(0), dt(1))
        r = qq - (o + ev * t[:, None])
        return t, _dot(r, r)
    t1, q1 = foot(a, ab, q)
    t2, q2 = foot(a, ac, q)
    t3, q3 = foot(b, c - b, q)
    g1, g2, best = t1, dt(0) * t1, q1
    m = q2 < best
    g1, g2, best = np.where(m, dt(0), g1), np.where(m, t2, g2), np.where(m, q2, best)
    m = q3 < best
    g1, g2 = np.where(m, dt(1) - t3, g1), np.where(m, t3, g2)
    b1, b2 = np.where(ok, b1, g1), np.where(ok, b2, g2)
    b0 = np.maximum((dt(1) - b1) - b2, dt(0))
    out = np.stack([b0, b1, b2], 1)
    assert out.dtype == q.dtype
    return out


def grads(P, V, F, g, dtype=np.float64):
    """the restatement: every operation in `dtype`.  g (N,) upstream gradient of the distance"""
    P, V, F, g = np.asarray(P, dtype), np.asarray(V, dtype), np.asarray(F), np.asarray(g, dtype)
    D, I, C = ref.mesh_distance_pruned(P, V, F, dtype)
    tri = F[I]
    bary = barycentric(P, V[tri[:, 0]], V[tri[:, 1]], V[tri[:, 2]])
    pos = D > 0
    n = (P - C) / np.where(pos, D, dtype(1))[:, None]
    dP = np.where(pos[:, None], g[:, None] * n, dtype(0))
    dV = np.zeros((len(V), 3), dtype)
    contrib = -(bary[:, :, None] * dP[:, None, :])               # (N, 3 corners, 3)
    np.add.at(dV, tri.reshape(-1), contrib.reshape(-1, 3))        # unbuffered, in index order: point 0 corner 0, 1, 2, point 1, ...
    assert dP.dtype == dtype and dV.dtype == dtype
    return dict(D=D, I=I, C=C, bary=bary, dP=dP, dV=dV)


def e32_dist(P, V, F):
    d64 = ref.mesh_distance_pruned(P, V, F, np.float64)[0]
    d32 = ref.mesh_distance_pruned(P, V, F, np.float32)[0]
    return float(np.abs(d32.astype(np.float64) - d64).max())


def all_pairs(P, V, F, chunk=64):
    """float64 distance (N,F) and closest point (N,F,3) of every point to every triangle"""
    P, V, F = np.asarray(P, np.float64), np.asarray(V, np.float64), np.asarray(F)
    a, b, c = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    D, Q = np.empty((len(P), len(F))), np.empty((len(P), len(F), 3))
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        q = ref.closest_point(p, a, b, c)
        Q[s:s + chunk], D[s:s + chunk] = q, np.sqrt(_dot(p - q, p - q))
    return D, Q


def ties(P, V, F, tol, chunk=64):
    """(N,) bool: some triangle whose closest point is farther than 1e-3 bounding-box diagonals of the mesh from the winner's
    lies within `tol` of the winning distance"""
    from scipy.spatial import cKDTree
    P, V, F = np.asarray(P, np.float64), np.asarray(V, np.float64), np.asarray(F)
    diag = float(np.linalg.norm(V.max(0) - V.min(0)))
    # only a triangle whose centroid lies within (winning distance + tol + largest triangle radius) can be that near
    # (the pruning of mesh_dist_ref.mesh_distance_pruned, widened by tol)
    tri = V[F]
    cen = tri.mean(1)
    rad = np.linalg.norm(tri - cen[:, None], axis=2).max(1).max()
    D, _, C = ref.mesh_distance_pruned(P, V, F)
    cands = cKDTree(cen).query_ball_point(P, D + tol + rad + 1e-9)
    out = np.zeros(len(P), bool)
    for s in range(0, len(P), chunk):
        idx = range(s, min(s + chunk, len(P)))
        cnt = np.array([len(cands[k]) for k in idx])
        fi = np.concatenate([np.asarray(cands[k], np.int64) for k in idx])
        pi = np.repeat(np.arange(idx.start, idx.stop), cnt)
        q = ref.closest_point(P[pi], V[F[fi, 0]], V[F[fi, 1]], V[F[fi, 2]])
        d = np.sqrt(_dot(P[pi] - q, P[pi] - q))
        hit = (np.linalg.norm(q - C[pi], axis=1) > 1e-3 * diag) & (d <= D[pi] + tol)
        out[np.unique(pi[hit])] = True
    return out


def fd_points(P, V, F, g, h=1e-6):
    """(N,3) central differences of sum_i g_i d_i with respect to the points (d_i depends on point i alone)"""
    P = np.asarray(P, np.float64)
    out = np.empty_like(P)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        out[:, k] = g * (ref.mesh_distance_pruned(P + e, V, F)[0] - ref.mesh_distance_pruned(P - e, V, F)[0]) / (2 * h)
    return out


def fd_verts(P, V, F, g, h=1e-6):
    """(V,3) central differences of sum_i g_i d_i with respect to the vertices.  A vertex moves only the triangles that use
    it: their columns of the all-pairs distance matrix are recomputed, the minimum over the others is kept"""
    P, V, F = np.asarray(P, np.float64), np.asarray(V, np.float64), np.asarray(F)
    D0 = all_pairs(P, V, F)[0]
    out = np.zeros_like(V)
    for v in range(len(V)):
        cols = np.nonzero((F == v).any(1))[0]
        if len(cols) == 0:
            continue
        rest = np.delete(D0, cols, axis=1).min(1) if len(cols) < len(F) else np.full(len(P), np.inf)
        for k in range(3):
            val = []
            for sgn in (1.0, -1.0):
                W = V.copy()
                W[v, k] += sgn * h
                t = W[F[cols]]
                q = ref.closest_point(P[:, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2])
                d = np.sqrt(_dot(P[:, None, :] - q, P[:, None, :] - q)).min(1)
                val.append((g * np.minimum(d, rest)).sum())
            out[v, k] = (val[0] - val[1]) / (2 * h)
    return out


# ---- the two spheres of the interpenetration tests: generic position, no exact ties (on the axis symmetry makes some) -------
def sphere_pair():
    """unit icosphere(2) at (0, 0, 2.2) and a radius-0.5 icosphere(2) at (1.13, 0.21, 2.37): (VA, FA, VB, FB), float32 values"""
    VA, FA = icosphere(2, 1.0, (0.0, 0.0, 2.2))
    VB, FB = icosphere(2, 0.5, (1.13, 0.21, 2.37))
    return (np.asarray(VA, np.float32).astype(np.float64), FA, np.asarray(VB, np.float32).astype(np.float64), FB)


def pen_loss(VA, FA, VB, dtype=np.float64):
    """sum_i inside_i dist_i / Vb of B's vertices in A, its gradient with respect to VB and VA, and the inside count"""
    import mesh_sign_ref as sref
    inside = np.abs(sref.winding(VB, VA, FA)) > 0.5
    r = grads(VB, VA, FA, inside.astype(np.float64) / len(VB), dtype)
    return float((r["D"].astype(np.float64) * inside).sum() / len(VB)), r["dP"], r["dV"], int(inside.sum())


def pair_loss(VA, FA, VB, FB, dtype=np.float64):
    """pen(A,B) + pen(B,A) and its gradient with respect to a translation of B -> (loss, (3,) gradient, (count, count))"""
    l1, dB1, _, c1 = pen_loss(VA, FA, VB, dtype)
    l2, _, dB2, c2 = pen_loss(VB, FB, VA, dtype)
    return l1 + l2, (dB1.astype(np.float64) + dB2.astype(np.float64)).sum(0), (c1, c2)


def descent(step=0.05, max_steps=8):
    """steps of `step` along the negative normalized gradient on the translation of the small sphere, float64 ->
    list of (loss, gradient, counts, translation)"""
    VA, FA, VB, FB = sphere_pair()
    t = np.zeros(3)
    hist = []
    for _ in range(max_steps + 1):
        loss, grad, cnt = pair_loss(VA, FA, VB + t, FB)
        hist.append((loss, grad, cnt, t.copy()))
        if loss == 0:
            break
        t = t - step * grad / np.linalg.norm(grad)
    return hist


# ---- the cases of tests/test_gpu_mesh_grad.py and tests/test_mesh_grad_host.py --------------------------------------------
BOX = ((-0.3, -0.2, 2.0), (0.4, 0.5, 2.6))
CASES = ("box12", "box1728", "ico2", "hemi", "body", "sphere_ab", "sphere_ba")
TIE_CAP = 0.01            # at most 1 % of a case's points may be left out as ties: a condition, not a measurement
SHARP = 1e-2              # the sharper comparison: points whose float64 distance is at least this


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def case_inputs(name):
    """(V, F, P) of a case: float64 arrays of float32 values"""
    import mesh_sign_ref as sref
    if name in ("box12", "box1728"):
        V, F = sref.oriented_box(BOX[0], BOX[1], 1 if name == "box12" else 12)
        P = (np.random.RandomState(1).rand(2400, 3) * 1.6 + np.array([-0.8, -0.7, 1.5]))[:600]      # the set of test_known_box
    elif name in ("ico2", "hemi"):
        ico = icosphere(2, 0.35, (0.45, 0.1, 2.3))
        V, F = ico if name == "ico2" else sref.hemisphere(2, 0.35, (0.45, 0.1, 2.3))
        P = ref.sampler_points([(f32(ico[0]), ico[1])], 170, 30, np.random.RandomState(0))[0]
    elif name == "body":
        from chore_amd.utils.synth import uv_ellipsoid
        V, F = uv_ellipsoid(center=(0.1, 0.2, 2.2))
        # 513 points, all of the sampler's surface kind (sigma 0.08 / 0.02 / 0.003) and none of its uniform ones.  A point d
        # from a mesh this fine (edges of 3 cm) has its foot point determined in float32 only to sqrt(2 d eps): 7e-4 m at d =
        # 2.4 m, 2 % of an edge, and so are the barycentric weights -- with the uniform points the restatement's own
        # E32(dV) is 2.4e-2, outside the (0, 1e-2) the comparisons require, and 11 of 513 count as ties (a triangle whose
        # closest point is 2 mm away is within 8 E32 of the winning distance: x^2 / 2d < 2e-6).  Near the surface: 0 ties.
        P = ref.sampler_points([(f32(V), F)], 171, 0, np.random.RandomState(2))[0]
    else:
        VA, FA, VB, FB = sphere_pair()
        V, F, P = (VA, FA, VB) if name == "sphere_ab" else (VB, FB, VA)
    return f32(V), np.asarray(F), f32(P)


def _e32(P, V, F, g):
    r64, r32 = grads(P, V, F, g), grads(P, V, F, g, np.float32)
    on = g != 0
    return r64, float(np.abs(r32["dP"].astype(np.float64) - r64["dP"])[on].max()), float(np.abs(r32["dV"].astype(np.float64) - r64["dV"]).max())


def make_case(name):
    """everything a comparison needs, computed once: the inputs, the upstream gradient g (0 on the points left out), the
    float64 restatement and E32 of dP and dV on the kept points, and the same for the sharper subset (g_sharp)"""
    V, F, P = case_inputs(name)
    E32d = e32_dist(P, V, F)
    tie = ties(P, V, F, 8 * E32d)
    w = f32(np.random.RandomState(5).uniform(0.5, 1.5, len(P)))
    g = np.where(tie, 0.0, w)
    r64, eP, eV = _e32(P, V, F, g)
    g_sharp = np.where(r64["D"] >= SHARP, g, 0.0)
    s64, sP, sV = _e32(P, V, F, g_sharp)
    return dict(name=name, V=V, F=F, P=P, E32_dist=E32d, tie=tie, g=g, r64=r64, E32_dP=eP, E32_dV=eV, g_sharp=g_sharp, s64=s64,
                E32_dP_sharp=sP, E32_dV_sharp=sV)
