"""The yardstick of the mesh-distance tests: the exact unsigned distance from points to a triangle mesh, restated with
numpy (+ scipy.spatial.cKDTree for an exact pruning), in float64 or, to measure what float32 arithmetic costs, in float32.

Contract (what np.abs(igl.signed_distance(P, V, F)[0]), its I and C mean): the minimum over all triangles of the
point-triangle distance.  Per triangle the closest point is found by the Voronoi regions of the triangle (vertex, edge,
interior; Ericson, Real-Time Collision Detection 5.1.5) with every division guarded, and -- because the region tests alone
send some points of a triangle with a repeated vertex to the wrong feature -- additionally on each of the three edges as a
segment; every candidate is a point of the triangle, the nearest one is taken.  A zero-area triangle is thereby the segment
or point it degenerates to.

    closest_point(p, a, b, c)        elementwise, any broadcastable (..., 3)
    mesh_distance_brute(P, V, F)     all pairs, chunked
    mesh_distance_pruned(P, V, F)    same numbers: only triangles whose centroid lies within (nearest referenced vertex
                                     distance + largest triangle radius) of the point can hold the closest point
    point_to_face(P, V, F, idx)      distance from point i to triangle idx[i]
    box_mesh / box_distance          a triangulated box and its closed-form distance
"""
import numpy as np
from scipy.spatial import cKDTree


def _dot(x, y):
    return (x * y).sum(-1)


def _sdiv(n, d):
    one = d.dtype.type(1)
    zero = d.dtype.type(0)
    ok = d != 0
    return np.where(ok, n / np.where(ok, d, one), zero)


def _segment(p, a, b):
    ab = b - a
    t = _sdiv(_dot(p - a, ab), _dot(ab, ab))
    t = np.minimum(np.maximum(t, t.dtype.type(0)), t.dtype.type(1))
    return a + ab * t[..., None]


def _voronoi(p, a, b, c):
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    denom = va + vb + vc
    v, w = _sdiv(vb, denom), _sdiv(vc, denom)
    q = a + ab * v[..., None] + ac * w[..., None]                    # interior
    zero = p.dtype.type(0) * p

    def put(mask, val):
        return np.where(mask[..., None], val, q)
    w_bc = _sdiv(d4 - d3, (d4 - d3) + (d5 - d6))
    q = put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + (c - b) * w_bc[..., None])
    q = put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * _sdiv(d2, d2 - d6)[..., None])
    q = put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * _sdiv(d1, d1 - d3)[..., None])
    q = put((d6 >= 0) & (d5 <= d6), c + zero)
    q = put((d3 >= 0) & (d4 <= d3), b + zero)
    q = put((d1 <= 0) & (d2 <= 0), a + zero)
    return q


def closest_point(p, a, b, c):
    """closest point of triangle (a, b, c) to p, all (..., 3) of one float dtype, broadcast against each other"""
    cands = [_voronoi(p, a, b, c), _segment(p, a, b), _segment(p, a, c), _segment(p, b, c)]
    best = cands[0]
    bd = _dot(p - best, p - best)
    for q in cands[1:]:
        d = _dot(p - q, p - q)
        m = d < bd
        best = np.where(m[..., None], q, best)
        bd = np.where(m, d, bd)
    return best


def point_to_face(P, V, F, idx, dtype=np.float64):
    """distance from P[i] to triangle F[idx[i]] and the closest point on it"""
    P, V = np.asarray(P, dtype), np.asarray(V, dtype)
    t = V[np.asarray(F)[np.asarray(idx)]]
    q = closest_point(P, t[:, 0], t[:, 1], t[:, 2])
    return np.sqrt(_dot(P - q, P - q)), q


def mesh_distance_brute(P, V, F, dtype=np.float64, chunk=256):
    """-> (D (N,), I (N,) first triangle attaining it, C (N,3) closest point), every point against every triangle"""
    P, V, F = np.asarray(P, dtype), np.asarray(V, dtype), np.asarray(F)
    a, b, c = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    D, I, C = np.empty(len(P), dtype), np.empty(len(P), np.int64), np.empty((len(P), 3), dtype)
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        q = closest_point(p, a, b, c)
        d2 = _dot(p - q, p - q)
        i = d2.argmin(1)
        r = np.arange(len(i))
        I[s:s + chunk], D[s:s + chunk], C[s:s + chunk] = i, np.sqrt(d2[r, i]), q[r, i]
    return D, I, C


def nearest_vertex(P, V):
    """float64 distance to and index of the nearest vertex"""
    d, i = cKDTree(np.asarray(V, np.float64)).query(np.asarray(P, np.float64))
    return d, i


def mesh_distance_pruned(P, V, F, dtype=np.float64, max_pairs=400_000):
    """the numbers of mesh_distance_brute from the candidate triangles only.  The candidate sets are found in float64 and
    are the same for both dtypes; the distances are evaluated in `dtype`."""
    P64, V64, F = np.asarray(P, np.float64), np.asarray(V, np.float64), np.asarray(F)
    tri = V64[F]
    cen = tri.mean(1)
    rad = np.linalg.norm(tri - cen[:, None], axis=2).max(1).max()
    ub, _ = nearest_vertex(P64, V64[np.unique(F)])               # a vertex of some triangle: an upper bound of the distance
    cands = cKDTree(cen).query_ball_point(P64, ub + rad + 1e-9)
    Pd, Vd = np.asarray(P, dtype), np.asarray(V, dtype)
    D, I, C = np.empty(len(P64), dtype), np.empty(len(P64), np.int64), np.empty((len(P64), 3), dtype)
    s = 0
    while s < len(P64):
        e, pairs = s, 0
        while e < len(P64) and (e == s or pairs + len(cands[e]) <= max_pairs):
            pairs += len(cands[e])
            e += 1
        cnt = np.array([len(cands[k]) for k in range(s, e)])
        fi = np.concatenate([np.sort(np.asarray(cands[k], np.int64)) for k in range(s, e)])
        pi = np.repeat(np.arange(s, e), cnt)
        p = Pd[pi]
        q = closest_point(p, Vd[F[fi, 0]], Vd[F[fi, 1]], Vd[F[fi, 2]])
        d2 = _dot(p - q, p - q)
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        dmin = np.minimum.reduceat(d2, start)
        first = np.minimum.reduceat(np.where(d2 == np.repeat(dmin, cnt), np.arange(len(d2)), len(d2)), start)
        D[s:e], I[s:e], C[s:e] = np.sqrt(dmin), fi[first], q[first]
        s = e
    return D, I, C


def box_mesh(lo, hi, n):
    """the surface of the box [lo, hi], every side an n x n grid of squares cut in two: 12 n^2 triangles"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    vs, fs, base = [], [], 0
    g = np.linspace(0.0, 1.0, n + 1)
    uu, ww = np.meshgrid(g, g, indexing="ij")
    for ax in range(3):
        u, w = [k for k in range(3) if k != ax]
        for side in (lo, hi):
            pts = np.zeros((n + 1, n + 1, 3))
            pts[..., ax] = side[ax]
            pts[..., u] = lo[u] + uu * (hi[u] - lo[u])
            pts[..., w] = lo[w] + ww * (hi[w] - lo[w])
            idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1) + base
            k0, k1, k2, k3 = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
            vs.append(pts.reshape(-1, 3))
            fs += [np.stack([k0, k1, k2], 1), np.stack([k0, k2, k3], 1)]
            base += (n + 1) ** 2
    return np.concatenate(vs), np.concatenate(fs).astype(np.int64)


def box_distance(P, lo, hi):
    """closed form: distance from P to the SURFACE of the box, for points outside and inside"""
    P, lo, hi = np.asarray(P, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = np.maximum(np.maximum(lo - P, P - hi), 0.0)
    inside = (out == 0).all(1)
    return np.where(inside, np.minimum(P - lo, hi - P).min(1), np.linalg.norm(out, axis=1))


def surface_samples(V, F, n, rs):
    """n area-weighted uniform surface points of the mesh from the numpy RandomState rs (float64)"""
    tri = np.asarray(V, np.float64)[np.asarray(F)]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    f = rs.choice(len(tri), n, p=area / area.sum())
    u = rs.rand(n, 2)
    m = u.sum(1) > 1
    u[m] = 1 - u[m]
    return tri[f, 0] + (tri[f, 1] - tri[f, 0]) * u[:, :1] + (tri[f, 2] - tri[f, 0]) * u[:, 1:]


BOUNDS = (np.array([-3.0, -0.9, 0.2]), np.array([3.0, 1.8, 4.0]))     # BoundarySampler.get_bounds()


def sampler_points(meshes, n_per_sigma, n_grid, rs, sigmas=(0.08, 0.02, 0.003)):
    """query points in the style of the sampler: per sigma, surface samples of the combined meshes + sigma N(0,1) and
    uniform points in BOUNDS, rounded to float32 (returned as float64 of those float32 values) -> (points, sigma id or -1)"""
    V = np.concatenate([m[0] for m in meshes])
    off = np.cumsum([0] + [len(m[0]) for m in meshes[:-1]])
    F = np.concatenate([m[1] + o for m, o in zip(meshes, off)])
    pts, tag = [], []
    for k, s in enumerate(sigmas):
        pts.append(surface_samples(V, F, n_per_sigma, rs) + s * rs.standard_normal((n_per_sigma, 3)))
        tag.append(np.full(n_per_sigma, k))
        pts.append(rs.rand(n_grid, 3) * (BOUNDS[1] - BOUNDS[0]) + BOUNDS[0])
        tag.append(np.full(n_grid, -1))
    return np.concatenate(pts).astype(np.float32).astype(np.float64), np.concatenate(tag)
