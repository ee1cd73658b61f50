"""Restatement (test infrastructure) of what chore_instances_fwd computes, in numpy, on top of the winners of the silhouette
restatement (render_ref.winners = oracle/silhouette.py), which are bit-equal to the kernels' winners.  Everything added on
top of winners is integer arithmetic, so every comparison with the kernel is exact.

Rule (include/chore_hip.h, chore_instances_fwd): the winner of a sample is the nearest candidate; vis_g = the winner's group is
g; full_g = some candidate has group g = the sub-list of group g's faces has a winner there; a face whose group lies outside
0..G-1 is an occluder: it wins samples and belongs to no group.  The resolve is render_ref.resolve's: the 2 x 2 samples added
in (row, column) order times 1/4, rows flipped.
"""
import numpy as np

import render_ref


F32 = np.float32


def winners_boxed(tri, S, near=0.1, far=100.0):
    """render_ref.winners for meshes of many faces: oracle/silhouette.py rasterize_fwd's expressions, operation for operation,
    evaluated for every face on the 16-aligned window around its box only (the kernels' own box: floor(min) - 1 .. ceil(max) + 1
    of the vertex pixel coordinates) and not on the whole image.  The kernels test a sample against a face only there, so for
    triangles with an area this is the same winner; tests/test_instances_host.py pins it against render_ref.winners."""
    tri = np.asarray(tri, F32)
    B, Fn = tri.shape[:2]
    Sf = F32(S)
    fim = -np.ones((B, S, S), np.int32)
    centre = ((2.0 * np.arange(S, dtype=np.float64) + 1 - S) / S).astype(F32)
    pix = np.arange(S, dtype=F32)
    for b in range(B):
        depth = np.full((S, S), far, F32)
        for fn in range(Fn):
            f = tri[b, fn].reshape(9)
            if (f[7] - f[1]) * (f[3] - f[0]) < (f[4] - f[1]) * (f[6] - f[0]):
                continue
            p = (F32(0.5) * (tri[b, fn, :, :2] * Sf + Sf - F32(1))).astype(F32)
            if not np.isfinite(p).all():
                continue
            x0, x1 = max(int(np.floor(p[:, 0].min())) - 1, 0), min(int(np.ceil(p[:, 0].max())) + 1, S - 1)
            y0, y1 = max(int(np.floor(p[:, 1].min())) - 1, 0), min(int(np.ceil(p[:, 1].max())) + 1, S - 1)
            if x0 > x1 or y0 > y1:
                continue
            x0, y0, x1, y1 = x0 & ~15, y0 & ~15, min(x1 | 15, S - 1), min(y1 | 15, S - 1)
            ys, xs = slice(y0, y1 + 1), slice(x0, x1 + 1)
            xp, yp, xi, yi = centre[None, xs], centre[ys, None], pix[None, xs], pix[ys, None]
            inv = np.array([p[1, 1] - p[2, 1], p[2, 0] - p[1, 0], p[1, 0] * p[2, 1] - p[2, 0] * p[1, 1],
                            p[2, 1] - p[0, 1], p[0, 0] - p[2, 0], p[2, 0] * p[0, 1] - p[0, 0] * p[2, 1],
                            p[0, 1] - p[1, 1], p[1, 0] - p[0, 0], p[0, 0] * p[1, 1] - p[1, 0] * p[0, 1]], F32)
            den = (p[2, 0] * (p[0, 1] - p[1, 1]) + p[0, 0] * (p[1, 1] - p[2, 1])) + p[1, 0] * (p[2, 1] - p[0, 1])
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = (inv / F32(den)).astype(F32)
                out = (((yp - f[1]) * (f[3] - f[0]) < (xp - f[0]) * (f[4] - f[1])) |
                       ((yp - f[4]) * (f[6] - f[3]) < (xp - f[3]) * (f[7] - f[4])) |
                       ((yp - f[7]) * (f[0] - f[6]) < (xp - f[6]) * (f[1] - f[7])))
                w = [np.clip((inv[3 * k] * xi + inv[3 * k + 1] * yi) + inv[3 * k + 2], F32(0), F32(1)).astype(F32)
                     for k in range(3)]
                ws = (w[0] + w[1]) + w[2]
                w = [wk / ws for wk in w]
                zp = F32(1) / ((w[0] / f[2] + w[1] / f[5]) + w[2] / f[8])
                hit = (~out) & ~((zp <= near) | (far <= zp)) & (zp < depth[ys, xs])
            depth[ys, xs] = np.where(hit, zp, depth[ys, xs]).astype(F32)
            fim[b, ys, xs] = np.where(hit, fn, fim[b, ys, xs])
    return fim


def pool(a, ssaa):
    """(B,G,S,S) per-sample 0/1 (rows not flipped) -> (B,G,S/ssaa,S/ssaa) float32 as the kernel resolves it"""
    a = a.astype(np.float32)
    if ssaa == 2:
        a = (((a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + a[..., 1::2, 0::2]) + a[..., 1::2, 1::2]) * np.float32(0.25)
    return np.ascontiguousarray(a[..., ::-1, :])


def instances(tri, face_group, G, size, ssaa, winners=render_ref.winners):
    """tri (B,F,3,3) float32, face_group (B,F) integers or None -> dict of visible, full (B,G,size,size) float32, face_samples
    (B,F) int32, group_samples (B,G,2) int32, face_index (B,S,S) int32 and the per-sample vis, cov (B,G,S,S) bool, S = size * ssaa.
    winners: render_ref.winners, or winners_boxed for meshes of many faces"""
    tri = np.asarray(tri, np.float32)
    B, Fn = tri.shape[:2]
    S = size * ssaa
    grp = np.zeros((B, Fn), np.int64) if face_group is None else np.asarray(face_group).astype(np.int64)
    fim = winners(tri, S)
    vis = np.zeros((B, G, S, S), bool)
    cov = np.zeros((B, G, S, S), bool)
    face_samples = np.zeros((B, Fn), np.int32)
    for b in range(B):
        won = fim[b] >= 0
        face_samples[b] = np.bincount(fim[b][won], minlength=Fn)
        wg = np.where(won, grp[b][np.maximum(fim[b], 0)], -1)
        for g in range(G):
            vis[b, g] = wg == g
            sel = np.nonzero(grp[b] == g)[0]
            if sel.size:
                cov[b, g] = winners(tri[b:b + 1, sel], S)[0] >= 0
    group_samples = np.stack([vis.sum((2, 3)), cov.sum((2, 3))], -1).astype(np.int32)
    return {"visible": pool(vis, ssaa), "full": pool(cov, ssaa), "face_samples": face_samples, "group_samples": group_samples,
            "face_index": fim, "vis": vis, "cov": cov}
