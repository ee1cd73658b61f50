"""CPU: the restatement of the renderer's backward (tests/render_bwd_ref.py) against the silhouette restatement, the
reference's own known answers (external/neural_renderer/tests/test_rasterize.py:84-156, test_rasterize_depth.py:57-90), and
the workspace query of chore_render_bwd."""
import os
import re

import numpy as np

import render_bwd_ref
import render_ref
from conftest import REPO
from render_bwd_cases import DEPTH_TRI, EYE, RGB_CASES
from oracle import silhouette as osil

def random_tri(seed, B=2, V=20, Fn=24):
    rs = np.random.RandomState(seed)
    v = np.concatenate([rs.uniform(-1.2, 1.2, (B, V, 2)), rs.uniform(0.5, 4.0, (B, V, 1))], -1).astype(np.float32)
    f = np.stack([np.stack([rs.choice(V, 3, replace=False) for _ in range(Fn)]) for _ in range(B)]).astype(np.int64)
    return osil.vertices_to_faces(v, osil.fill_back(f)), rs


def doubled(verts):
    """one triangle with both windings as fill_back lists them: (1,2,3,3), and the fold of its gradient back to the vertices"""
    v = np.asarray(verts, np.float32)
    return np.stack([v, v[::-1]])[None]


def fold(g_tri):
    return g_tri[0, 0] + g_tri[0, 1][::-1]


def test_alpha_only_equals_the_silhouette_restatement():
    """with the rgb and depth upstream gradients zero, in float32, the walk is oracle.silhouette.rasterize_bwd's bit for bit"""
    tri, rs = random_tri(3)
    B, Fn = tri.shape[:2]
    S = 32
    fim, alpha = osil.rasterize_fwd(tri, S)
    assert 0.05 < (fim >= 0).mean() < 0.95
    g = rs.standard_normal((B, S, S)).astype(np.float32)
    want = osil.rasterize_bwd(tri, fim, alpha, g, eps=osil.EPS)
    tex = rs.uniform(0, 1, (B, Fn, 2, 2, 2, 3)).astype(np.float32)
    got = render_bwd_ref.render_bwd(tri, tex, None, fim, 1, np.zeros((B, 3, S, S), np.float32), np.zeros((B, S, S), np.float32),
                                    g[:, ::-1], eps=osil.EPS, background=(0.2, 0.3, 0.4), dtype=np.float32)
    assert np.abs(want).max() > 1
    assert np.array_equal(got["tri"], want)
    assert not got["textures"].any() and not got["light"].any() and not got["depth"].any()


def rgb_case_gradient(verts, pix, minus_one, dtype=np.float64):
    tri = doubled(np.asarray(verts, np.float32) - EYE)
    fim = render_ref.winners(tri, 64)
    tex = np.ones((1, 2, 2, 2, 2, 3), np.float32)
    light = np.ones((1, 2, 3), np.float32)                       # ambient 1, directional 0
    rgb, _, _ = render_ref.render(tri, tex, light, fim, 1, tex_eps=1e-3, dtype=dtype)
    image = rgb[0].mean(0)
    g = np.zeros((1, 3, 64, 64), dtype)
    g[0, :, pix[0], pix[1]] = np.sign(image[pix] - (1 if minus_one else 0)) / 3
    zero = np.zeros((1, 64, 64), dtype)
    return fold(render_bwd_ref.render_bwd(tri, tex, light, fim, 1, g, zero, zero, eps=1e-3, dtype=dtype)["tri"])


def test_reference_rgb_known_answers():
    """the two analytic vectors of test_rasterize.py (white texture, mean over the channels) at that test's own rtol"""
    for verts, pix, minus_one, ref in RGB_CASES:
        got = rgb_case_gradient(verts, pix, minus_one)
        print(got)
        np.testing.assert_allclose(got, np.array(ref), rtol=1e-2, atol=1e-6)


def depth_loss(verts, dtype):
    tri = doubled(verts)
    fim = render_ref.winners(tri, 64)
    _, depth, _ = render_ref.render(tri, np.ones((1, 2, 2, 2, 2, 3), np.float32), None, fim, 1, dtype=dtype)
    return (depth[0, 15, 20] - 1) ** 2, tri, fim, depth


def depth_case(dtype=np.float64):
    """-> (analytic gradient (3,3) of the restatement, forward differences of the restatement's forward)"""
    v = np.array(DEPTH_TRI, np.float32)
    loss, tri, fim, depth = depth_loss(v, dtype)
    g = np.zeros((1, 64, 64), dtype)
    g[0, 15, 20] = 2 * (depth[0, 15, 20] - 1)
    grad = fold(render_bwd_ref.render_bwd(tri, np.ones((1, 2, 2, 2, 2, 3), np.float32), None, fim, 1, None, g, None, dtype=dtype)["tri"])
    fd = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            v2 = v.copy()
            v2[i, j] += np.float32(1e-3)
            fd[i, j] = (depth_loss(v2, dtype)[0] - loss) / 1e-3
    return grad, fd


def test_reference_depth_finite_differences():
    """the reference's own criterion for the depth rule: forward differences of step 1e-3, atol 1e-3.  Measured on the
    float64 restatement: the largest deviation is 9.1e-4, on z of the nearest vertex (the curvature of the loss over the step: forward differences are first order; rounding is far below)"""
    grad, fd = depth_case()
    print("analytic\n", grad, "\nforward differences\n", fd, "\nlargest deviation", np.abs(grad - fd).max())
    assert np.abs(grad).max() > 0.1
    np.testing.assert_allclose(grad, fd, rtol=0, atol=1e-3)


def test_texture_and_light_sum_to_the_colour_gradient():
    """the taps' weights sum to one and the light is a factor: sum over the texels of grad_textures = light x the summed rgb
    gradient of the face's samples, and grad_light of a uniformly coloured face = that colour x the summed rgb gradient"""
    tri, rs = random_tri(5)
    B, Fn = tri.shape[:2]
    fim = render_ref.winners(tri, 48)
    colour = rs.uniform(0.1, 1, (B, Fn, 3)).astype(np.float32)
    tex = np.broadcast_to(colour[:, :, None, None, None, :], (B, Fn, 3, 3, 3, 3)).copy()
    light = rs.uniform(0.3, 1, (B, Fn, 3)).astype(np.float32)
    g = rs.standard_normal((B, 3, 24, 24))
    out = render_bwd_ref.render_bwd(tri, tex, light, fim, 2, g, None, None)
    gs = render_bwd_ref.upstream_to_samples(g.transpose(0, 2, 3, 1), 2, np.float64)
    per_face = np.zeros((B, Fn, 3))
    for b in range(B):
        hit = fim[b] >= 0
        np.add.at(per_face[b], fim[b][hit], gs[b][hit])
    assert np.abs(per_face).max() > 0.1
    assert np.abs(out["textures"].sum((2, 3, 4)) - light * per_face).max() < 1e-12
    assert np.abs(out["light"] - colour * per_face).max() < 1e-12


def test_render_bwd_workspace_bytes():
    """callable without a GPU; from the shapes alone; 0 = unsupported; header, ctypes and the library agree"""
    from chore_amd import _lib
    ws = _lib.lib.chore_render_bwd_workspace_bytes
    base = ws(3, 80, 2, 24, 2)
    assert base >= 3 * 48 * 48 * 36 + 3 * 80 * 88
    assert ws(3, 80, 2, 24, 3) == 0 and ws(3, 80, 2, 24, 0) == 0
    assert ws(1, 80, 2, 2049, 2) == 0 and ws(1, 80, 2, 4097, 1) == 0 and ws(1, 80, 2, 2048, 2) > 0
    assert ws(3, 80, 1, 24, 2) == 0 and ws(0, 80, 2, 24, 2) == 0 and ws(3, 0, 2, 24, 2) == 0
    assert ws(3, 160, 2, 24, 2) > base and ws(3, 80, 2, 48, 2) > base and ws(6, 80, 2, 24, 2) > base
    assert ws(3, 80, 4, 24, 2) == base                                   # texels are accumulated in registers
    hdr = open(os.path.join(REPO, "include", "chore_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"size_t\s+chore_render_bwd_workspace_bytes\s*\(\s*int B, int F, int ts, int size, int ssaa\s*\)", hdr)
    assert re.search(r"int\s+chore_render_bwd\s*\(", hdr)
    res, args = _lib.SIGNATURES["chore_render_bwd"]
    assert len(args) == 23 and hasattr(_lib.lib, "chore_render_bwd")
