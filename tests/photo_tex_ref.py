"""Restatement (test infrastructure) of what chore_photo_textures_fwd and chore_point_visibility compute, in float64 numpy,
written from the rule in include/chore_hip.h.  The depth image is GIVEN (the library's own, or a host restatement's), so the
rasteriser's winners never enter a comparison.

Besides the values it returns the texels a comparison with a float32 evaluation leaves out, each for a stated reason: a float32
position of magnitude <= 64 carries an error near 1e-5, so a decision that hangs on less than the margins below may fall either
way in float32 and says nothing about the rule.
  sample   px + 0.5 or py + 0.5 within SAMPLE_MARGIN of an integer: the nearest sample (or in view / out of view) is undecided
  depth    |z - depth - bias| < DEPTH_MARGIN at the chosen sample
  near     |z - near| < DEPTH_MARGIN
  photo    for visible texels, qx or qy within PHOTO_MARGIN of an edge of the photo
"""
import numpy as np

SAMPLE_MARGIN = PHOTO_MARGIN = 1e-3
DEPTH_MARGIN = 1e-4


def texel_weights(ts):
    """(ts,ts,ts,3) float64: w = (i,j,k) / (i+j+k), (1/3,1/3,1/3) for the texel (0,0,0)"""
    ijk = np.stack(np.meshgrid(np.arange(ts), np.arange(ts), np.arange(ts), indexing="ij"), -1).astype(np.float64)
    n = ijk.sum(-1, keepdims=True)
    w = ijk / np.where(n > 0, n, 1.0)
    w[0, 0, 0] = 1.0 / 3.0
    return w


def seen(u, v, z, depth_b, near, far, bias):
    """steps 2, 4 and 5 on arrays u, v, z of one image against its (S,S) depth image (rows not flipped)
    -> (in_range, in_view, visible, left_out) bool arrays"""
    S = depth_b.shape[0]
    with np.errstate(invalid="ignore"):
        in_range = (near < z) & (z < far)
        px, py = 0.5 * ((u * S + S) - 1.0), 0.5 * ((v * S + S) - 1.0)
        tx, ty = px + 0.5, py + 0.5
        xi, yi = np.floor(tx), np.floor(ty)
        in_view = in_range & (xi >= 0) & (xi <= S - 1) & (yi >= 0) & (yi <= S - 1)
        xs = np.where(in_view, xi, 0).astype(np.int64)
        ys = np.where(in_view, yi, 0).astype(np.int64)
        d = depth_b.astype(np.float64)[ys, xs]
        visible = in_view & (z <= d + bias)
        edge = (np.abs(tx - np.round(tx)) < SAMPLE_MARGIN) | (np.abs(ty - np.round(ty)) < SAMPLE_MARGIN)
        left = (np.abs(z - near) < DEPTH_MARGIN) | (in_range & edge) | (in_view & (np.abs(z - d - bias) < DEPTH_MARGIN))
    return in_range, in_view, visible, left


def photo_position(u, v, Hp, Wp, align_corners):
    """step 6 -> (qx, qy, in_photo, near_edge)"""
    with np.errstate(invalid="ignore"):
        if align_corners:
            qx, qy = (u + 1.0) * 0.5 * (Wp - 1.0), (1.0 - v) * 0.5 * (Wp - 1.0)
        else:
            qx, qy = 0.5 * ((u * Wp + Wp) - 1.0), 0.5 * (((-v) * Wp + Wp) - 1.0)
        inside = (-0.5 <= qx) & (qx <= Wp - 0.5) & (-0.5 <= qy) & (qy <= Hp - 0.5)
        edge = np.zeros(np.shape(qx), bool)
        for q, e in ((qx, -0.5), (qx, Wp - 0.5), (qy, -0.5), (qy, Hp - 0.5)):
            edge |= np.abs(q - e) < PHOTO_MARGIN
    return qx, qy, inside, edge


def bilinear(photo_b, qx, qy):
    """the four taps around (qx, qy) of a (3,Hp,Wp) photo, tap indices clamped -> (..., 3)"""
    Hp, Wp = photo_b.shape[1:]
    x0, y0 = np.floor(qx), np.floor(qy)
    fx, fy = (qx - x0)[..., None], (qy - y0)[..., None]
    xa, xb = np.clip(x0, 0, Wp - 1).astype(np.int64), np.clip(x0 + 1, 0, Wp - 1).astype(np.int64)
    ya, yb = np.clip(y0, 0, Hp - 1).astype(np.int64), np.clip(y0 + 1, 0, Hp - 1).astype(np.int64)
    p = np.moveaxis(photo_b.astype(np.float64), 0, -1)              # (Hp,Wp,3)
    top = p[ya, xa] * (1 - fx) + p[ya, xb] * fx
    bot = p[yb, xa] * (1 - fx) + p[yb, xb] * fx
    return top * (1 - fy) + bot * fy


def photo_textures(tri, depth, photo, fallback, ts, near=0.1, far=100.0, bias=0.02, align_corners=False):
    """tri (B,F,3,3), depth (B,S,S), photo (B,3,Hp,Wp), fallback (B,F,3) -> dict of (B,F,ts,ts,ts[,3]) arrays:
    textures float64, visible, left_out, and the classes in_view, in_photo (visible and in the photo) as bool"""
    tri = np.asarray(tri, np.float32).astype(np.float64)
    photo = np.asarray(photo, np.float32)
    fallback = np.asarray(fallback, np.float32).astype(np.float64)
    B, Fn = tri.shape[:2]
    Hp, Wp = photo.shape[2:]
    w = texel_weights(ts)                                           # (ts,ts,ts,3)
    shape = (B, Fn, ts, ts, ts)
    out = {"textures": np.empty(shape + (3,)), "visible": np.empty(shape, bool), "left_out": np.empty(shape, bool),
           "in_view": np.empty(shape, bool), "in_photo": np.empty(shape, bool)}
    for b in range(B):
        uk, vk, zk = (tri[b, :, :, d][:, None, None, None, :] for d in range(3))           # (F,1,1,1,3)
        with np.errstate(invalid="ignore", divide="ignore"):
            z = (w[..., 0] * zk[..., 0] + w[..., 1] * zk[..., 1]) + w[..., 2] * zk[..., 2]
            s = (w * zk) / z[..., None]
            u = (s[..., 0] * uk[..., 0] + s[..., 1] * uk[..., 1]) + s[..., 2] * uk[..., 2]
            v = (s[..., 0] * vk[..., 0] + s[..., 1] * vk[..., 1]) + s[..., 2] * vk[..., 2]
        _, in_view, vis, left = seen(u, v, z, np.asarray(depth[b]), near, far, bias)
        qx, qy, inside, edge = photo_position(np.where(vis, u, 0.0), np.where(vis, v, 0.0), Hp, Wp, align_corners)
        use = vis & inside
        colour = bilinear(photo[b], np.where(use, qx, 0.0), np.where(use, qy, 0.0))
        out["textures"][b] = np.where(use[..., None], colour, fallback[b][:, None, None, None, :])
        out["visible"][b], out["in_view"][b], out["in_photo"][b] = vis, in_view, use
        out["left_out"][b] = left | (vis & edge)
    return out


def point_visibility(pts, depth, near=0.1, far=100.0, bias=0.02):
    """pts (B,N,3), depth (B,S,S) -> (visible (B,N) bool, left_out (B,N) bool)"""
    pts = np.asarray(pts, np.float32).astype(np.float64)
    res = [seen(p[:, 0], p[:, 1], p[:, 2], np.asarray(d), near, far, bias) for p, d in zip(pts, depth)]
    return np.stack([r[2] for r in res]), np.stack([r[3] for r in res])


# ---- the inputs of test 1, shared by the host and the GPU test

CASES = ((64, 4), (61, 2), (61, 5))         # (S, ts): a grid that is no multiple of a tile, the smallest cube, an odd cube
LEFT_OUT_CAP = 0.02                         # at most this share of the texels of any image may be left out
BIAS = 0.02


def random_inputs(tri):
    """photo (3,3,48,64) in [0,1]: a quarter of the square is outside the photo; fallback (3,F,3) in [0,1]"""
    rs = np.random.RandomState(1)
    return rs.uniform(0, 1, (tri.shape[0], 3, 48, 64)).astype(np.float32), rs.uniform(0, 1, tri.shape[:2] + (3,)).astype(np.float32)


def random_tri(seed=0, B=3, V=30, Fn=40):
    """random_tri of tests/test_gpu_instances.py: projected triangles in and around the view, small triangles in image 1,
    degenerate vertices in image 2, both windings (face f + Fn is face f the other way round)"""
    from oracle import silhouette as osil
    rs = np.random.RandomState(seed)
    v = np.concatenate([rs.uniform(-1.2, 1.2, (B, V, 2)), rs.uniform(0.5, 4.0, (B, V, 1))], -1).astype(np.float32)
    f = np.stack([np.stack([rs.choice(V, 3, replace=False) for _ in range(Fn)]) for _ in range(B)]).astype(np.int64)
    v[1, :, :2] *= 0.3
    v[2, :5] = 0.0
    return osil.vertices_to_faces(v, osil.fill_back(f))


def host_depth(tri, S, far=100.0):
    """the depth image on the host: the silhouette restatement's winners and the float64 depth rule, rounded to float32"""
    import ordinal_depth_ref
    import render_ref
    return ordinal_depth_ref.winner_depth(tri, render_ref.winners(tri, S), far=far, flip=False)[0].astype(np.float32)


def shares(ref):
    """per image: the share of texels in view, visible, occluded (in view, not visible), visible but outside the photo, left out"""
    ax = tuple(range(1, ref["visible"].ndim))
    return {"in_view": ref["in_view"].mean(ax), "visible": ref["visible"].mean(ax),
            "occluded": (ref["in_view"] & ~ref["visible"]).mean(ax), "outside_photo": (ref["visible"] & ~ref["in_photo"]).mean(ax),
            "left_out": ref["left_out"].mean(ax)}
