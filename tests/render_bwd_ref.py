"""Restatement (test infrastructure) of chore_render_bwd in numpy, in the dtype asked for (float64, or float32 in the order
of the CUDA source), on top of tests/render_ref.py: the winning face per sample is GIVEN, as there.

Rules (external/neural_renderer/neural_renderer/rasterize.py:114-170, 319-340 and cuda/rasterize_cuda_kernel.cu):
  upstream     the gradient of output pixel (r, x), divided by ssaa^2, goes to each of its samples in sample row block
               size-1-r: the transpose of the flip and of F.avg_pool2d
  pixel map    :290-549, per face, edge and axis: walk the samples the edge crosses; 'out' samples beyond the edge and 'in'
               samples up to the opposite edge contribute diff_grad / distance to the two edge vertices, diff_grad = the
               alpha contribution + the three rgb contributions, gated by diff_grad <= 0 AFTER the sum
  textures     :551-586: the eight taps of the forward's sampling, weight x rgb gradient (x light, which the reference
               multiplies into the textures beforehand); light: rgb gradient x the blended texel
  depth        :588-638 on the winner of every hit sample: d z_k = g w_k d^2 / z_k^2, d (x, y)_k = -g tmp_l w_k d^2 S / 2 with
               tmp_l = sum_m -inv[3 m + l] / z_m
Per-sample colours are the forward's: tests/render_ref.py sample_values.
"""
import numpy as np

import render_ref


def upstream_to_samples(g, ssaa, dtype):
    """g (B,s,s[,..]) rows flipped, as the renderer returns them -> (B,S,S) per sample, rows not flipped, divided by ssaa^2"""
    g = np.asarray(g).astype(dtype)[:, ::-1]
    if ssaa == 2:
        g = np.repeat(np.repeat(g, 2, axis=1), 2, axis=2) * np.dtype(dtype).type(0.25)
    return np.ascontiguousarray(g)


def _backside(f):
    return (f[7] - f[1]) * (f[3] - f[0]) < (f[4] - f[1]) * (f[6] - f[0])


def minus(acc, values):
    """acc - values[0] - values[1] - ...: one by one in float32 (the order of the CUDA source), in one go in float64"""
    if values.dtype == np.float64:
        return acc - values.sum()
    for v in values:
        acc = acc - v
    return acc


def pixel_map_bwd(tri, fim, rgb, alpha, g_rgb, g_alpha, eps, dtype):
    """tri (B,F,3,3); per-sample fim (B,S,S), rgb (B,S,S,3), alpha (B,S,S) and their gradients (None = not returned by the
    forward, like return_rgb / return_alpha = False) -> grad_tri (B,F,3,3) in `dtype` (depth components zero)"""
    T = np.dtype(dtype).type
    tri = np.asarray(tri, np.float32).astype(dtype)
    B, Fn = tri.shape[:2]
    size = fim.shape[1]
    S = T(size)
    eps = T(np.float32(eps))
    out = np.zeros((B, Fn, 9), dtype)
    for b in range(B):
        M = fim[b]
        # one (S,S,C) value image and its gradient: alpha first, then rgb, the order diff_grad is summed in
        chans, grads = [], []
        if g_alpha is not None:
            chans.append(alpha[b][..., None]); grads.append(g_alpha[b][..., None])
        if g_rgb is not None:
            chans.append(rgb[b]); grads.append(g_rgb[b])
        V = np.concatenate(chans, -1).astype(dtype)
        G = np.concatenate(grads, -1).astype(dtype)

        def line(axis, d0, lo, hi):          # the samples (d0, lo..hi) of a scan line: values, gradients, winners
            if axis == 0:
                return V[lo:hi + 1, d0], G[lo:hi + 1, d0], M[lo:hi + 1, d0]
            return V[d0, lo:hi + 1], G[d0, lo:hi + 1], M[d0, lo:hi + 1]

        def at(axis, d0, d1):
            return (d1, d0) if axis == 0 else (d0, d1)

        for fn in range(Fn):
            f = tri[b, fn].reshape(9)
            if _backside(f):
                continue
            gf = np.zeros(9, dtype)
            for e in range(3):
                pi = [(e + k) % 3 for k in range(3)]
                pp = np.array([[T(0.5) * (f[3 * pi[k] + d] * S + S - T(1)) for d in range(2)] for k in range(3)], dtype)
                for axis in range(2):
                    p = pp[:, [axis, 1 - axis]]
                    if axis == 0:
                        direction = -1 if p[0, 0] < p[1, 0] else 1
                    else:
                        direction = 1 if p[0, 0] < p[1, 0] else -1
                    lo0, hi0 = min(p[0, 0], p[1, 0]), max(p[0, 0], p[1, 0])
                    if not (np.isfinite(lo0) and np.isfinite(hi0)):
                        continue
                    d0_from = int(max(np.ceil(lo0), 0.0))
                    d0_to = int(min(hi0, size - 1.0))
                    for d0 in range(d0_from, d0_to + 1):
                        fd0 = T(d0)
                        with np.errstate(divide="ignore", invalid="ignore"):
                            cross = T((p[1, 1] - p[0, 1]) / (p[1, 0] - p[0, 0]) * (fd0 - p[0, 0]) + p[0, 1])
                        if not np.isfinite(cross):
                            continue
                        d1_in = int(np.floor(cross)) if direction > 0 else int(np.ceil(cross))
                        d1_out = d1_in + direction
                        if not (0 <= d1_in < size and 0 <= d1_out < size):
                            continue
                        v_in, v_out = V[at(axis, d0, d1_in)], V[at(axis, d0, d1_out)]

                        def push(lo, hi, ref, own):
                            vals, grads_, faces_ = line(axis, d0, lo, hi)
                            diff = np.zeros(hi - lo + 1, dtype)
                            for c in range(vals.shape[1]):
                                diff = diff + (vals[:, c] - ref[c]) * grads_[:, c]
                            take = diff > 0
                            if own:
                                take &= faces_ == fn
                            if not take.any():
                                return
                            d1 = np.arange(lo, hi + 1)[take].astype(dtype)
                            diff = diff[take]
                            with np.errstate(divide="ignore", invalid="ignore"):
                                if p[1, 0] != fd0:
                                    dist = (p[1, 0] - p[0, 0]) / (p[1, 0] - fd0) * (d1 - cross) * T(2) / S
                                    dist = np.where(dist > 0, dist + eps, dist - eps)
                                    gf[pi[0] * 3 + (1 - axis)] = minus(gf[pi[0] * 3 + (1 - axis)], diff / dist)
                                if p[0, 0] != fd0:
                                    dist = (p[1, 0] - p[0, 0]) / (fd0 - p[0, 0]) * (d1 - cross) * T(2) / S
                                    dist = np.where(dist > 0, dist + eps, dist - eps)
                                    gf[pi[1] * 3 + (1 - axis)] = minus(gf[pi[1] * 3 + (1 - axis)], diff / dist)

                        if M[at(axis, d0, d1_in)] == fn:        # 'out'
                            lim = size - 1 if direction > 0 else 0
                            push(max(min(d1_out, lim), 0), min(max(d1_out, lim), size - 1), v_in, False)
                        with np.errstate(divide="ignore", invalid="ignore"):
                            if (fd0 - p[0, 0]) * (fd0 - p[2, 0]) < 0:
                                c2 = (p[2, 1] - p[0, 1]) / (p[2, 0] - p[0, 0]) * (fd0 - p[0, 0]) + p[0, 1]
                            else:
                                c2 = (p[1, 1] - p[2, 1]) / (p[1, 0] - p[2, 0]) * (fd0 - p[2, 0]) + p[2, 1]
                        if not np.isfinite(c2):
                            continue
                        lim = int(np.ceil(c2)) if direction > 0 else int(np.floor(c2))
                        lo, hi = max(min(d1_in, lim), 0), min(max(d1_in, lim), size - 1)
                        if lo <= hi:
                            push(lo, hi, v_out, True)
            out[b, fn] = gf
    return out.reshape(B, Fn, 3, 3)


def _winner_terms(tri, b, fim, dtype):
    """for the hit samples of image b: (yi, xi, fn, weights [3 x (n,)], zp (n,), inv (n,9), z [3 x (n,)])"""
    T = np.dtype(dtype).type
    S = fim.shape[1]
    Sf = T(S)
    yi, xi = np.nonzero(fim[b] >= 0)
    fn = fim[b, yi, xi]
    f = tri[b, fn]
    p = T(0.5) * ((f[:, :, :2] * Sf + Sf) - T(1))
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
    return yi, xi, fn, w, zp, inv, z


def depth_bwd(tri, fim, g_depth, dtype):
    """per-sample depth gradient (B,S,S) -> grad_tri (B,F,3,3)"""
    T = np.dtype(dtype).type
    tri = np.asarray(tri, np.float32).astype(dtype)
    B, Fn = tri.shape[:2]
    S = fim.shape[1]
    out = np.zeros((B, Fn, 3, 3), dtype)
    for b in range(B):
        if not (fim[b] >= 0).any():
            continue
        yi, xi, fn, w, zp, inv, z = _winner_terms(tri, b, fim, dtype)
        g = g_depth[b, yi, xi].astype(dtype)
        d2 = zp * zp
        tmp = [-(inv[:, l] / z[0] + inv[:, 3 + l] / z[1] + inv[:, 6 + l] / z[2]) for l in range(2)]
        for k in range(3):
            np.add.at(out[b, :, k, 2], fn, g * w[k] * d2 / (z[k] * z[k]))
            for l in range(2):
                np.add.at(out[b, :, k, l], fn, -g * tmp[l] * w[k] * d2 * T(S) / T(2))
    return out


def texture_light_bwd(tri, textures, light, fim, g_rgb, tex_eps, dtype):
    """per-sample rgb gradient (B,S,S,3) -> grad_textures (B,F,ts,ts,ts,3), grad_light (B,F,3)"""
    T = np.dtype(dtype).type
    tri = np.asarray(tri, np.float32).astype(dtype)
    tex = np.asarray(textures, np.float32).astype(dtype)
    B, Fn = tri.shape[:2]
    ts = tex.shape[2]
    lt = np.ones((B, Fn, 3), dtype) if light is None else np.asarray(light, np.float32).astype(dtype)
    g_tex = np.zeros(tex.shape, dtype)
    g_light = np.zeros((B, Fn, 3), dtype)
    for b in range(B):
        if not (fim[b] >= 0).any():
            continue
        yi, xi, fn, w, zp, _, z = _winner_terms(tri, b, fim, dtype)
        g = g_rgb[b, yi, xi].astype(dtype)                       # (n,3)
        tmax = T(ts - 1) - T(np.float32(tex_eps))
        tif = [np.clip((w[k] * T(ts - 1)) * (zp / z[k]), T(0), tmax) for k in range(3)]
        ti = [t.astype(np.int64) for t in tif]
        fr = [tif[k] - ti[k].astype(dtype) for k in range(3)]
        blended = np.zeros((yi.size, 3), dtype)
        for pn in range(8):
            wt = np.ones(yi.size, dtype)
            idx = []
            for k in range(3):
                up = (pn >> k) & 1
                wt = wt * (fr[k] if up else T(1) - fr[k])
                idx.append(np.minimum(ti[k] + up, ts - 1))
            blended = blended + wt[:, None] * tex[b, fn, idx[0], idx[1], idx[2]]
            np.add.at(g_tex[b], (fn, idx[0], idx[1], idx[2]), wt[:, None] * (g * lt[b, fn]))
        np.add.at(g_light[b], fn, g * blended)
    return g_tex, g_light


def render_bwd(tri, textures, light, fim, ssaa, g_rgb, g_depth, g_alpha, near=0.1, far=100.0, tex_eps=1e-3, eps=1e-3,
               background=(0, 0, 0), dtype=np.float64):
    """what chore_render_bwd computes: upstream gradients as the renderer's outputs are laid out (g_rgb (B,3,s,s), g_depth and
    g_alpha (B,s,s), each may be None) -> dict(tri (B,F,3,3) = pixel map + depth, pixel_map, depth, textures, light)"""
    tri32 = np.asarray(tri, np.float32)
    B, Fn = tri32.shape[:2]
    rgb, _, alpha = render_ref.sample_values(tri32, textures, light, fim, near, far, tex_eps, background, dtype)
    s_rgb = None if g_rgb is None else upstream_to_samples(np.asarray(g_rgb).transpose(0, 2, 3, 1), ssaa, dtype)
    s_depth = None if g_depth is None else upstream_to_samples(g_depth, ssaa, dtype)
    s_alpha = None if g_alpha is None else upstream_to_samples(g_alpha, ssaa, dtype)
    out = {"pixel_map": np.zeros((B, Fn, 3, 3), dtype), "depth": np.zeros((B, Fn, 3, 3), dtype),
           "textures": np.zeros(np.asarray(textures).shape, dtype), "light": np.zeros((B, Fn, 3), dtype)}
    if s_rgb is not None or s_alpha is not None:
        out["pixel_map"] = pixel_map_bwd(tri32, fim, rgb, alpha, s_rgb, s_alpha, eps, dtype)
    if s_depth is not None:
        out["depth"] = depth_bwd(tri32, fim, s_depth, dtype)
    if s_rgb is not None:
        out["textures"], out["light"] = texture_light_bwd(tri32, textures, light, fim, s_rgb, tex_eps, dtype)
    out["tri"] = out["pixel_map"] + out["depth"]
    return out
