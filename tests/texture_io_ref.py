"""float64 numpy restatement of chore_load_textures and chore_texture_atlas (csrc/texture_io.hip), written from the rules in
include/chore_hip.h, with the case tables and the left-out rule of tests/test_gpu_texture_io.py.  Only the wrap of step 4 is done
in float32, operation by operation, so that it is the same number on both sides; everything after it is float64."""
import numpy as np

WRAPS = {'REPEAT': 0, 'MIRRORED_REPEAT': 1, 'CLAMP_TO_EDGE': 2, 'CLAMP_TO_BORDER': 3}
LOAD_CASES = [(1, 2, 1, 1), (5, 2, 5, 7), (37, 4, 48, 64), (37, 5, 33, 17), (300, 4, 64, 64)]      # F, ts, H, W
UV_RANGE = {'REPEAT': (-2.5, 3.5), 'MIRRORED_REPEAT': (-2.5, 3.5), 'CLAMP_TO_EDGE': (-0.1, 1.1)}
LOAD_TOL = 1e-4           # position error <= 2e-5 px at W <= 64, slope <= 1 per px and axis for values in [0,1], fp32 rounding on top
HALF_MARGIN = 2e-4        # nearest: a position this close (px) to a half-integer may round either way
LEFT_OUT_CAP = 0.02       # of a case; a condition on the case, not a tolerance
ATLAS_F, ATLAS_TSI, ATLAS_TSO = (1, 2, 5, 10), (2, 4), (2, 3, 16)
ATLAS_TOL = 2e-5          # weights to 2 ulp x (tsi-1 <= 15) x slope <= 1 per axis x 3 axes, plus the blend
EPS = 1e-5


def second_image_size(H, W):
    """the second image of a load case: another size, still at most 64 px on a side"""
    return max(W - 1, 1) if W > 1 else 2, max(H - 2, 1)


def load_inputs(F, ts, H, W, wrap, seed=0):
    """uv (F,3,2) float32 uniform in the wrap's range, face_image (F): of every five faces three on image 0, one on image 1 (of
    another size) and one colour-only, face_color (F,3) float32, images [(H,W,3), (H2,W2,3)] uint8"""
    rng = np.random.default_rng(1000 * seed + 7 * F + ts + H + W + WRAPS[wrap])
    lo, hi = UV_RANGE.get(wrap, (-2.5, 3.5))
    uv = rng.uniform(lo, hi, (F, 3, 2)).astype(np.float32)
    face_image = np.asarray([(0, 0, 0, 1, -1)[f % 5] for f in range(F)], np.int32)
    face_color = rng.uniform(0, 1, (F, 3)).astype(np.float32)
    H2, W2 = second_image_size(H, W)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H2, W2, 3), dtype=np.uint8)]
    return uv, face_image, face_color, images


def _mod32(x, y):
    """mod(x,y) = x > 0 ? fmodf(x,y) : y + fmodf(x,y), float32"""
    y = np.float32(y)
    r = np.fmod(x, y).astype(np.float32)
    return np.where(x > 0, r, (y + r).astype(np.float32)).astype(np.float32)


def wrap32(x, mode):
    """step 4 on a float32 array, each operation rounded to float32"""
    x = np.asarray(x, np.float32)
    if mode == 0:
        return _mod32(x, 1)
    if mode == 1:
        m1 = _mod32(x, 1)
        return np.where(_mod32(x, 2) < 1, m1, (np.float32(1) - m1).astype(np.float32)).astype(np.float32)
    return np.minimum(np.maximum(x, np.float32(0)), np.float32(1)).astype(np.float32)


def texel_weights(ts):
    """step 3 -> (ts,ts,ts,3) float64"""
    g = np.stack(np.meshgrid(*(np.arange(ts, dtype=np.float64),) * 3, indexing="ij"), -1) / (ts - 1)
    s = g.sum(-1, keepdims=True)
    return np.where(s > 0, g / np.where(s > 0, s, 1), g)


def load_textures(uv, face_image, face_color, images, ts, wrapping, bilinear):
    """-> dict(textures (F,ts,ts,ts,3) float64, left_out (F,ts,ts,ts) bool: nearest texels within HALF_MARGIN of a half-integer
    position, sampled (F,) bool: the faces that took their texels from an image)"""
    F = len(uv)
    out = np.broadcast_to(np.asarray(face_color, np.float64)[:, None, None, None, :], (F, ts, ts, ts, 3)).copy()
    left_out = np.zeros((F, ts, ts, ts), bool)
    sampled = np.zeros(F, bool)
    d = texel_weights(ts)
    finite = np.isfinite(np.asarray(uv, np.float32)).reshape(F, 6).all(1)
    for m, img in enumerate(images):
        sel = np.nonzero((np.asarray(face_image) == m))[0]
        if not len(sel):
            continue
        if wrapping == 3:
            out[sel] = 0.0
            continue
        sel = sel[finite[sel]]
        if not len(sel):
            continue
        sampled[sel] = True
        H, W = img.shape[:2]
        flipped = img[::-1].astype(np.float64) / 255.0
        w = wrap32(np.asarray(uv, np.float32)[sel], wrapping).astype(np.float64)                     # (n,3,2)
        px = np.einsum("nc,ijkc->nijk", w[:, :, 0], d) * (W - 1)
        py = np.einsum("nc,ijkc->nijk", w[:, :, 1], d) * (H - 1)
        if bilinear:
            xi, yi = np.trunc(px).astype(np.int64), np.trunc(py).astype(np.int64)
            fx, fy = (px - xi)[..., None], (py - yi)[..., None]
            x0, y0 = np.clip(xi, 0, W - 1), np.clip(yi, 0, H - 1)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            top = flipped[y0, x0] + (flipped[y0, x1] - flipped[y0, x0]) * fx
            bot = flipped[y1, x0] + (flipped[y1, x1] - flipped[y1, x0]) * fx
            out[sel] = top + (bot - top) * fy
        else:
            x0 = np.clip(np.floor(px + 0.5).astype(np.int64), 0, W - 1)            # positions are >= 0: half away from zero
            y0 = np.clip(np.floor(py + 0.5).astype(np.int64), 0, H - 1)
            out[sel] = flipped[y0, x0]
            near_half = lambda p: np.abs(p - np.floor(p) - 0.5) < HALF_MARGIN      # noqa: E731
            left_out[sel] = near_half(px) | near_half(py)
    return {"textures": out, "left_out": left_out, "sampled": sampled}


def atlas_tiles(F):
    """integer tile counts -> (tile_w, tile_h)"""
    import math
    tile_w = math.isqrt(F - 1) + 1
    return tile_w, (F - 1) // tile_w + 1


def _trilinear(cubes, fn, w, tsi):
    """cubes (F,tsi,tsi,tsi,3) float64, fn (...) face per pixel, w (...,3) weights -> (...,3), step 5"""
    t = np.minimum(np.maximum(w * (tsi - 1), 0.0), tsi - 1 - EPS)
    lo = t.astype(np.int64)
    fr = t - lo
    hi = np.minimum(lo + 1, tsi - 1)
    out = np.zeros(fn.shape + (3,))
    for a in range(2):
        for b in range(2):
            for c in range(2):
                idx = [(hi if bit else lo)[..., q] for q, bit in enumerate((a, b, c))]
                wt = np.prod([(fr if bit else 1 - fr)[..., q] for q, bit in enumerate((a, b, c))], axis=0)
                out += wt[..., None] * cubes[fn, idx[0], idx[1], idx[2]]
    return out


def texture_atlas(textures, tso):
    """textures (F,tsi,tsi,tsi,3) -> image (tile_h tso, tile_w tso, 3) float64 in file row order.  The weights are computed in
    tile-local coordinates AND by the reference's general formula (the barycentric coordinates of the pixel in the tile triangle
    p0 = tile corner, p1 = p0 + (0,T), p2 = p0 + (T,T), over (sum + eps)); the two are asserted equal."""
    cubes = np.asarray(textures, np.float64)
    F, tsi = cubes.shape[:2]
    tile_w, tile_h = atlas_tiles(F)
    Hh, Ww, T = tile_h * tso, tile_w * tso, tso - 1
    y, x = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")                # y counted from the bottom
    col, row = x // tso, y // tso
    fn = col + row * tile_w
    lx, ly = x % tso, y % tso
    shift = (ly + 1 == lx)
    lx = lx - shift
    w_local = np.stack([(T - ly) / T, (ly - lx) / T, lx / T], -1) / (1 + EPS)
    # the general formula at the (shifted) global position
    gx, gy = (x - shift).astype(np.float64), y.astype(np.float64)
    p0 = np.stack([col * tso, row * tso], -1).astype(np.float64)
    p1, p2 = p0 + [0, T], p0 + [T, T]
    den = p2[..., 0] * (p0[..., 1] - p1[..., 1]) + p0[..., 0] * (p1[..., 1] - p2[..., 1]) + p1[..., 0] * (p2[..., 1] - p0[..., 1])

    def bary(a, b):            # the coordinate that is 1 at the third vertex: the line through a and b, normalised
        return ((a[..., 1] - b[..., 1]) * gx + (b[..., 0] - a[..., 0]) * gy + (a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1])) / den
    w_global = np.stack([bary(p1, p2), bary(p2, p0), bary(p0, p1)], -1)
    w_global = w_global / (w_global.sum(-1, keepdims=True) + EPS)
    assert np.abs(w_global - w_local).max() < 1e-12, np.abs(w_global - w_local).max()
    exists = fn < F
    image = np.where(exists[..., None], _trilinear(cubes, np.where(exists, fn, 0), w_local, tsi), 0.0)
    return image[::-1].copy()
