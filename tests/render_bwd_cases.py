"""The cases of tests/test_gpu_render_bwd.py (test infrastructure): triangles, textures, light and upstream gradients, built
the same way on every machine so that the seeds can be chosen without a GPU (see `leave_out`)."""
import math

import numpy as np

from oracle import silhouette as osil

NEAR, FAR, TEX_EPS, EPS = 0.1, 100.0, 1e-3, 1e-3
BG = (0.3, 0.2, 0.7)

EYE = np.array([0, 0, -(1.0 / math.tan(math.radians(30)) + 1)], np.float32)      # Renderer(camera_mode='look_at').eye

# test_rasterize.py:84-156: vertices, (pyi, pxi), the loss is |x - 1| (True) or |x| (False), grad_ref
RGB_CASES = [
    ([[0.8, 0.8, 1.], [0.0, -0.5, 1.], [0.2, -0.4, 1.]], (25, 35), True,
     [[1.6725862, -0.26021874, 0.], [1.41986704, -1.64284933, 0.], [0., 0., 0.]]),
    ([[0.8, 0.8, 1.], [-0.5, -0.8, 1.], [0.8, -0.8, 1.]], (40, 50), False,
     [[0.98646867, 1.04628897, 0.], [-1.03415668, -0.10403691, 0.], [3.00094461, -1.55173182, 0.]]),
]
# test_rasterize_depth.py:57-90: camera_mode 'none', pixel (15, 20), loss (d - 1)^2, forward differences of step 1e-3
DEPTH_TRI = [[-0.9, -0.9, 2.], [-0.8, 0.8, 1.], [0.8, 0.8, 0.5]]


def _finish(tri, rs, ts, size, ssaa):
    B, Fn = tri.shape[:2]
    return dict(tri=np.ascontiguousarray(tri, np.float32), tex=rs.uniform(0, 1, (B, Fn, ts, ts, ts, 3)).astype(np.float32),
                light=rs.uniform(0.3, 1.0, (B, Fn, 3)).astype(np.float32), size=size, ssaa=ssaa,
                g_rgb=rs.standard_normal((B, 3, size, size)).astype(np.float32),
                g_depth=rs.standard_normal((B, size, size)).astype(np.float32),
                g_alpha=rs.standard_normal((B, size, size)).astype(np.float32))


def random_case(seed, ts, size, ssaa, B=3, V=30, Fn=40):
    """B images of Fn triangles doubled by fill_back (so half of them are back faces): vertices in and around the view, small
    triangles in image 1, repeated vertices (zero-area triangles) in image 2, and in every image vertices in front of near
    and beyond far"""
    rs = np.random.RandomState(seed)
    v = np.concatenate([rs.uniform(-1.2, 1.2, (B, V, 2)), rs.uniform(0.5, 4.0, (B, V, 1))], -1).astype(np.float32)
    f = np.stack([np.stack([rs.choice(V, 3, replace=False) for _ in range(Fn)]) for _ in range(B)]).astype(np.int64)
    if B > 2:
        v[1, :, :2] *= 0.3
        v[2, :5] = v[2, 0]
    v[:, 5, 2] = 0.05
    v[:, 6, 2] = 150.0
    f[:, 0] = (7, 7, 8)                                   # a zero-area face in every image
    return _finish(osil.vertices_to_faces(v, osil.fill_back(f)), rs, ts, size, ssaa)


def tie_case(seed=21):
    """two coplanar faces at equal depth (the same triangle twice: the smaller index wins every sample) among others"""
    c = random_case(seed, 2, 32, 1, B=1, V=12, Fn=8)
    tri = c["tri"]
    tri[0, 3] = tri[0, 1] = np.array([[-0.6, -0.5, 1.0], [0.7, -0.3, 1.0], [0.1, 0.8, 1.0]], np.float32)
    tri[0, 8 + 3] = tri[0, 8 + 1] = tri[0, 1][::-1]
    return c


def large_face_case(seed=22):
    """one triangle over most of a 32 px image at 2x beside tiny ones in front of it: one workgroup sums thousands of samples"""
    rs = np.random.RandomState(seed)
    big = np.array([[-1.8, -0.95, 3.0], [1.9, -0.9, 2.0], [0.05, 2.2, 2.5]], np.float32)
    c = rs.uniform(-0.8, 0.8, (10, 1, 2))
    small = np.concatenate([c + rs.uniform(-0.08, 0.08, (10, 3, 2)), rs.uniform(0.8, 1.5, (10, 3, 1))], -1).astype(np.float32)
    tri = np.concatenate([big[None], small])
    tri = np.concatenate([tri, tri[:, ::-1]])[None]
    return _finish(tri, rs, 3, 32, 2)


def multi_bin_case(seed=23):
    """size 136 at 2x: 272 samples, more than one coarse bin of the forward and tail tiles, 16 triangles"""
    return random_case(seed, 2, 136, 2, B=1, V=10, Fn=8)


def leave_out(r32, r64, bound):
    """the faces whose pixel-map gradient the float32 restatement itself does not reproduce: (B,F) bool"""
    return np.abs(r32.astype(np.float64) - r64).reshape(r64.shape[:2] + (-1,)).max(-1) > bound
