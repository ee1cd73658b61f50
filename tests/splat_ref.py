"""numpy restatement of the splat rule of chore_splat_fwd (include/chore_hip.h), parameterised by dtype.

Points are visited in ascending index and take a sample with a strict `<` on depth, so the winner of a sample is the covering
point with the smallest depth, then the smallest index.  Every operation is one numpy operation on `dtype` values in the
association the header writes down: with float32 this reproduces the kernel's winners bit for bit, with float64 it is the
yardstick for the values.  The inputs are the float32 numbers the kernel sees, converted to `dtype` without change.
"""
import numpy as np

MAX_RS = 64.0


def splat_samples(pts, colors, radius, S, ssaa, ambient, near, far, background, dtype=np.float32):
    """pts (B,N,3), colors (B,N,3) or None, radius (B,N) in output pixels or a scalar -> per sample, rows not flipped:
    index (B,S,S) int32 (-1 = none), rgb (B,S,S,3), depth (B,S,S), alpha (B,S,S) in `dtype`"""
    f = dtype
    pts = np.asarray(pts, np.float32)
    B, N = pts.shape[:2]
    per_point = np.ndim(radius) > 0
    rad = np.asarray(radius, np.float32)
    Sf, amb, near, far = f(S), f(np.float32(ambient)), f(np.float32(near)), f(np.float32(far))
    bg = np.asarray(background, np.float32).astype(f)
    index = np.full((B, S, S), -1, np.int32)
    zb = np.full((B, S, S), far, f)
    d2b = np.zeros((B, S, S), f)
    rs2b = np.ones((B, S, S), f)
    with np.errstate(all="ignore"):
        for b in range(B):
            for n in range(N):
                u, v, z = (f(c) for c in pts[b, n])
                r = f(rad[b, n]) if per_point else f(rad)
                if np.isnan(u) or np.isnan(v) or np.isnan(z) or np.isnan(r):
                    continue
                if r <= 0 or z <= near or far <= z:
                    continue
                rs = min(r * f(ssaa), f(MAX_RS))
                px = f(0.5) * ((u * Sf + Sf) - f(1.0))
                py = f(0.5) * ((v * Sf + Sf) - f(1.0))
                # a generous box (two samples of slack) only saves work; the test below decides
                lo_x, hi_x = np.floor(float(px) - float(rs)) - 2, np.ceil(float(px) + float(rs)) + 2
                lo_y, hi_y = np.floor(float(py) - float(rs)) - 2, np.ceil(float(py) + float(rs)) + 2
                if not (np.isfinite(lo_x) and np.isfinite(hi_x) and np.isfinite(lo_y) and np.isfinite(hi_y)):
                    continue
                x0, x1, y0, y1 = int(max(lo_x, 0)), int(min(hi_x, S - 1)), int(max(lo_y, 0)), int(min(hi_y, S - 1))
                if x0 > x1 or y0 > y1:
                    continue
                dx = np.arange(x0, x1 + 1).astype(f) - px
                dy = np.arange(y0, y1 + 1).astype(f) - py
                d2 = (dx * dx)[None, :] + (dy * dy)[:, None]
                rs2 = rs * rs
                win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
                take = (d2 <= rs2) & (z < zb[b][win])
                if take.any():
                    index[b][win][take] = n
                    zb[b][win][take] = z
                    d2b[b][win][take] = d2[take]
                    rs2b[b][win][take] = rs2
        hit = index >= 0
        shade = amb + (f(1.0) - amb) * np.sqrt(np.maximum(f(0.0), f(1.0) - d2b / rs2b))
        if colors is None:
            col = np.ones((B, S, S, 3), f)
        else:
            c = np.asarray(colors, np.float32).astype(f)
            col = np.stack([c[b][np.maximum(index[b], 0)] for b in range(B)])
        rgb = np.where(hit[..., None], col * shade[..., None], bg[None, None, None, :]).astype(f)
    return index, rgb, zb, hit.astype(f)


def resolve(x, ssaa):
    """sample rows not flipped (B,S,S[,C]) -> output pixels (B,size,size[,C]): the mean over the ssaa x ssaa samples summed
    in the kernel's order (row by row, starting from 0), then the row flip"""
    acc = np.zeros_like(x[:, 0::ssaa, 0::ssaa])
    for sy in range(ssaa):
        for sx in range(ssaa):
            acc = acc + x[:, sy::ssaa, sx::ssaa]
    return (acc * x.dtype.type(1.0 / (ssaa * ssaa)))[:, ::-1]


def splat(pts, colors, radius, size, ssaa, ambient=0.6, near=0.1, far=100.0, background=(0, 0, 0), dtype=np.float32):
    """the whole call: dict(index (B,S,S) rows not flipped, rgb (B,3,size,size), depth, alpha (B,size,size)) in `dtype`"""
    S = size * ssaa
    index, rgb, depth, alpha = splat_samples(pts, colors, radius, S, ssaa, ambient, near, far, background, dtype)
    return {"index": index, "rgb": np.ascontiguousarray(resolve(rgb, ssaa).transpose(0, 3, 1, 2)),
            "depth": resolve(depth, ssaa), "alpha": resolve(alpha, ssaa)}


def pixels_agree(index_a, index_b, ssaa):
    """(B,size,size) bool, rows flipped like the outputs: every sample of the pixel has the same winner in both maps"""
    same = index_a == index_b
    ok = np.ones_like(same[:, 0::ssaa, 0::ssaa])
    for sy in range(ssaa):
        for sx in range(ssaa):
            ok &= same[:, sy::ssaa, sx::ssaa]
    return ok[:, ::-1]


NEAR, FAR = 0.1, 100.0


def issue_cloud(seed, B=3, N=300, ssaa=2):
    """the seeded clouds of the winner tests: u, v ~ U(-1.15, 1.15), z ~ U(0.05, 3), radii 0.3 + 5.7 U^4 SAMPLES (0.3 .. 6, mostly
    small, so that some samples stay empty even at 32^2; returned in output pixels), colours on the 1/256 grid, plus the special points (fixed indices, every image):
      0..3  far outside the frame (one overflows u * S)       4..7  centred on each border, 4 samples radius
      8     z == near      9   z == far      10  NaN u       11  NaN radius     12  radius 0     13  radius < 0
      14, 250   identical position, depth and radius (14 must win wherever either does)
      20    4 samples radius at z = 1        21  2 samples radius right behind it at z = 2 (never visible)
    -> pts (B,N,3), colors (B,N,3), radius (B,N) float32"""
    rs = np.random.RandomState(seed)
    pts = np.concatenate([rs.uniform(-1.15, 1.15, (B, N, 2)), rs.uniform(0.05, 3.0, (B, N, 1))], -1).astype(np.float32)
    rad = ((0.3 + 5.7 * rs.uniform(0.0, 1.0, (B, N)) ** 4) / ssaa).astype(np.float32)
    col = (rs.randint(32, 256, (B, N, 3)) / 256.0).astype(np.float32)
    pts[:, 0] = (3.0, 0.1, 1.0)
    pts[:, 1] = (0.2, -2.5, 1.0)
    pts[:, 2] = (-1e38, 0.0, 1.0)
    pts[:, 3] = (np.inf, 0.3, 1.0)
    for k, uv in enumerate(((-1.0, 0.1), (1.0, -0.3), (0.4, -1.0), (-0.6, 1.0))):
        pts[:, 4 + k, :2] = uv
        rad[:, 4 + k] = 4.0 / ssaa
    pts[:, 8, 2] = np.float32(NEAR)
    pts[:, 9, 2] = np.float32(FAR)
    pts[:, 10, 0] = np.nan
    rad[:, 11] = np.nan
    rad[:, 12] = 0.0
    rad[:, 13] = -1.5
    pts[:, 250] = pts[:, 14] = (0.31, -0.22, 0.9)
    rad[:, 250] = rad[:, 14] = 3.0 / ssaa
    pts[:, 20] = (-0.4, 0.45, 1.0)
    pts[:, 21] = (-0.4, 0.45, 2.0)
    rad[:, 20], rad[:, 21] = 4.0 / ssaa, 2.0 / ssaa
    return pts, col, rad


# (size, ssaa) of the winner / value tests
ISSUE_GRIDS = ((32, 1), (32, 2), (33, 2))
