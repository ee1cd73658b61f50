"""Restatement (test infrastructure) of what chore_render_fwd computes per sample and of its resolve, in numpy, in the
dtype asked for (float32 in the kernel's operation order, or float64), on top of the silhouette restatement
oracle/silhouette.py: the winning face per sample is GIVEN (oracle.silhouette.rasterize_fwd's, or the kernel's own
sample_face_index), so a tie between two faces can never enter a comparison of values.

Rule (external/neural_renderer/neural_renderer/cuda/rasterize_cuda_kernel.cu:161-177, 255-287; rasterize.py:62, 319-340):
weights w = clamp(inv * (xi, yi, 1), 0, 1) / sum, zp = 1 / sum(w_k / z_k); texture index tif_k = clamp(w_k (ts-1) (zp / z_k),
0, ts-1-eps); colour = trilinear blend of the 8 neighbouring texels of the face's ts^3 cube, times the per-face light;
background colour / far / 0 where no face won; then rows flipped and, for ssaa = 2, the mean of the 2x2 samples.
"""
import numpy as np

from oracle import silhouette as osil


def winners(tri, S):
    """(B,S,S) int32 winning face per sample at image size S (rows not flipped): the silhouette restatement"""
    return osil.rasterize_fwd(tri, S)[0]


def sample_values(tri, textures, light, fim, near, far, tex_eps, background, dtype):
    """per-sample rgb (B,S,S,3), depth (B,S,S), alpha (B,S,S) in `dtype` for the winners `fim` (B,S,S)"""
    T = np.dtype(dtype).type
    tri = np.asarray(tri, np.float32).astype(dtype)
    tex = np.asarray(textures, np.float32).astype(dtype)
    B, Fn = tri.shape[:2]
    ts = tex.shape[2]
    S = fim.shape[1]
    Sf = T(S)
    rgb = np.empty((B, S, S, 3), dtype)
    rgb[...] = np.asarray(background, np.float32).astype(dtype)
    depth = np.full((B, S, S), T(np.float32(far)), dtype)
    alpha = (fim >= 0).astype(dtype)
    for b in range(B):
        yi, xi = np.nonzero(fim[b] >= 0)
        if yi.size == 0:
            continue
        fn = fim[b, yi, xi]
        f = tri[b, fn]                                            # (n,3,3)
        p = T(0.5) * ((f[:, :, :2] * Sf + Sf) - T(1))             # pixel coordinates of the vertices
        den = (p[:, 2, 0] * (p[:, 0, 1] - p[:, 1, 1]) + p[:, 0, 0] * (p[:, 1, 1] - p[:, 2, 1])) + p[:, 1, 0] * (p[:, 2, 1] - p[:, 0, 1])
        m = np.stack([p[:, 1, 1] - p[:, 2, 1], p[:, 2, 0] - p[:, 1, 0], p[:, 1, 0] * p[:, 2, 1] - p[:, 2, 0] * p[:, 1, 1],
                      p[:, 2, 1] - p[:, 0, 1], p[:, 0, 0] - p[:, 2, 0], p[:, 2, 0] * p[:, 0, 1] - p[:, 0, 0] * p[:, 2, 1],
                      p[:, 0, 1] - p[:, 1, 1], p[:, 1, 0] - p[:, 0, 0], p[:, 0, 0] * p[:, 1, 1] - p[:, 1, 0] * p[:, 0, 1]], 1)
        inv = (m / den[:, None]).astype(dtype)
        xf, yf = xi.astype(dtype), yi.astype(dtype)
        w = [np.clip((inv[:, 3 * k] * xf + inv[:, 3 * k + 1] * yf) + inv[:, 3 * k + 2], T(0), T(1)) for k in range(3)]
        ws = (w[0] + w[1]) + w[2]
        w = [wk / ws for wk in w]
        z = [f[:, k, 2] for k in range(3)]
        zp = T(1) / ((w[0] / z[0] + w[1] / z[1]) + w[2] / z[2])
        assert np.all((zp > T(np.float32(near))) & (zp < T(np.float32(far)))), "a winner outside near / far"
        tmax = T(ts - 1) - T(np.float32(tex_eps))
        tif = [np.clip((w[k] * T(ts - 1)) * (zp / z[k]), T(0), tmax) for k in range(3)]
        ti = [t.astype(np.int64) for t in tif]
        fr = [tif[k] - ti[k].astype(dtype) for k in range(3)]
        c = np.zeros((yi.size, 3), dtype)
        cube = tex[b, fn]                                          # (n,ts,ts,ts,3)
        n = np.arange(yi.size)
        for pn in range(8):
            wt = np.ones(yi.size, dtype)
            idx = []
            for k in range(3):
                up = (pn >> k) & 1
                wt = wt * (fr[k] if up else T(1) - fr[k])
                idx.append(np.minimum(ti[k] + up, ts - 1))
            c = c + wt[:, None] * cube[n, idx[0], idx[1], idx[2]]
        if light is not None:
            c = c * np.asarray(light, np.float32).astype(dtype)[b, fn]
        rgb[b, yi, xi] = c
        depth[b, yi, xi] = zp
    return rgb, depth, alpha


def resolve(rgb, depth, alpha, ssaa):
    """per-sample images (rows not flipped) -> what the renderer returns: rgb (B,3,s,s), depth, alpha (B,s,s); the samples
    of a pixel are added in the order (row, column) of the un-flipped sample image, then multiplied by 1 / ssaa^2"""
    T = rgb.dtype.type

    def pool(a):                 # a (B,S,S[,3]), rows not flipped
        if ssaa == 1:
            out = a
        else:
            out = (((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + a[:, 1::2, 0::2]) + a[:, 1::2, 1::2]) * T(0.25)
        return out[:, ::-1]
    return np.ascontiguousarray(pool(rgb).transpose(0, 3, 1, 2)), np.ascontiguousarray(pool(depth)), np.ascontiguousarray(pool(alpha))


def render(tri, textures, light, fim, ssaa, near=0.1, far=100.0, tex_eps=1e-3, background=(0, 0, 0), dtype=np.float64):
    return resolve(*sample_values(tri, textures, light, fim, near, far, tex_eps, background, dtype), ssaa)
