"""CPU: the float64 restatement of the photo-texture rule (tests/photo_tex_ref.py) against analytic colours, and the share of
texels its comparison leaves out on the inputs of tests/test_gpu_photo_textures.py, so the cap is checked where no GPU is needed."""
import numpy as np
import pytest

import photo_tex_ref as pref


def _ramp(Hp, Wp):
    """photo (1,3,Hp,Wp) whose channels are linear in (x, y): a bilinear blend reproduces it exactly between the tap centres"""
    y, x = np.meshgrid(np.arange(Hp, dtype=np.float64), np.arange(Wp, dtype=np.float64), indexing="ij")
    coef = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.5, 3.0]])            # channel = a x + b y + c
    return np.stack([a * x + b * y + c for a, b, c in coef])[None].astype(np.float32), coef


@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("ts", [2, 4, 5])
def test_fronto_parallel_triangle_on_a_ramp(ts, align_corners):
    """one triangle at constant depth 2 in front of nothing: every texel is visible, sits at sum w_k (u_k, v_k) and takes the
    ramp's value at its photo position; one metre behind a wall every texel takes the fallback"""
    Hp, Wp, S = 48, 64, 32
    uv = np.array([[-0.5, 0.75], [0.25, 0.5], [-0.125, 0.125]])                       # inside the photo's upper part (v > -0.5 + margin)
    tri = np.concatenate([uv, np.full((3, 1), 2.0)], 1)[None, None].astype(np.float32)
    photo, coef = _ramp(Hp, Wp)
    fallback = np.array([[[0.1, 0.2, 0.3]]], np.float32)
    ref = pref.photo_textures(tri, np.full((1, S, S), 2.0, np.float32), photo, fallback, ts, align_corners=align_corners)
    assert ref["visible"].all() and ref["in_photo"].all()
    w = pref.texel_weights(ts)
    u, v = w @ uv[:, 0], w @ uv[:, 1]
    if align_corners:
        qx, qy = (u + 1) * 0.5 * (Wp - 1), (1 - v) * 0.5 * (Wp - 1)
    else:
        qx, qy = ((u + 1) * Wp - 1) / 2, ((1 - v) * Wp - 1) / 2
    assert qx.min() > 0 and qx.max() < Wp - 1 and qy.min() > 0 and qy.max() < Hp - 1
    want = coef[:, 0] * qx[..., None] + coef[:, 1] * qy[..., None] + coef[:, 2]
    assert np.abs(ref["textures"][0, 0] - want).max() < 1e-10
    assert np.array_equal(w[ts - 1, 0, 0], [1, 0, 0]) and np.array_equal(w[0, ts - 1, 0], [0, 1, 0]) and np.array_equal(w[0, 0, ts - 1], [0, 0, 1])
    hidden = pref.photo_textures(tri, np.full((1, S, S), 1.0, np.float32), photo, fallback, ts, align_corners=align_corners)
    assert not hidden["visible"].any() and hidden["in_view"].all()
    assert np.array_equal(hidden["textures"], np.broadcast_to(fallback.astype(np.float64)[:, :, None, None, None], hidden["textures"].shape))


def test_rows_and_the_photo_edge():
    """v = +1 is the photo's top edge and the square's lower part does not exist: a texel at v < 1 - 2 Hp / Wp is visible but takes the
    fallback; point_visibility is the texel rule on the vertices"""
    Hp, Wp, S = 48, 64, 16
    photo = np.zeros((1, 3, Hp, Wp), np.float32)
    photo[:, :, :2] = 1.0                                                              # the two top rows are white
    tri = np.array([[[[0.0, 0.98, 2.0], [0.02, 0.98, 2.0], [0.0, 0.96, 2.0]], [[0.0, -0.7, 2.0], [0.1, -0.7, 2.0], [0.0, -0.8, 2.0]]]], np.float32)
    fallback = np.full((1, 2, 3), 0.5, np.float32)
    depth = np.full((1, S, S), 100.0, np.float32)
    ref = pref.photo_textures(tri, depth, photo, fallback, 2)
    assert ref["visible"].all() and ref["in_photo"][0, 0].all() and not ref["in_photo"][0, 1].any()
    assert ref["textures"][0, 0].min() == 1.0 and np.array_equal(np.unique(ref["textures"][0, 1]), [0.5])
    vis, _ = pref.point_visibility(tri.reshape(1, 6, 3), depth)
    assert vis.all()
    assert not pref.point_visibility(tri.reshape(1, 6, 3) + np.float32([2.0, 0, 0]), depth)[0].any()          # out of view


@pytest.mark.parametrize("S,ts", pref.CASES)
def test_left_out_share_is_within_the_cap(S, ts):
    """the comparison of tests/test_gpu_photo_textures.py leaves out at most 2 % of the texels of any image, and every class of
    texel is populated (the depth image here is the host restatement's; the GPU test takes the library's)"""
    tri = pref.random_tri(0)
    photo, fallback = pref.random_inputs(tri)
    depth = pref.host_depth(tri, S)
    for align_corners in (False, True):
        ref = pref.photo_textures(tri, depth, photo, fallback, ts, bias=pref.BIAS, align_corners=align_corners)
        sh = pref.shares(ref)
        print(S, ts, align_corners, {k: np.round(v, 4).tolist() for k, v in sh.items()})
        assert (sh["left_out"] <= pref.LEFT_OUT_CAP).all()
        # every class is populated in every image, but for two that image 1 cannot have: its triangles are scaled into
        # |u|, |v| < 0.36, so all of them are in view and inside the photo's rows (v > -0.5)
        assert all((sh[k] > 0).all() for k in ("in_view", "visible", "occluded"))
        assert (sh["outside_photo"][[0, 2]] > 0).all() and (sh["in_view"][[0, 2]] < 1).all()
