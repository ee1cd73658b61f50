"""CPU: the layered composite rule of tests/scene_layers_ref.py -- equal to tests/scene_ref.py with one group, and one hand case
per clause -- plus render_utils.mesh_face_group and the signatures that grew the face_layers / face_group keywords."""
import inspect

import numpy as np
import pytest

import scene_layers_ref
import scene_ref

F32 = np.float32
BG = np.array([0.25, 0.5, 0.75], F32)
FAR = 100.0
M = np.array([[0.8, 0.4, 0.2], [0.2, 0.9, 0.3], [0.6, 0.1, 0.7], [0.3, 0.3, 0.9]], F32)      # the layers' colours
P = np.array([0.1, 0.6, 0.9], F32)                                                            # the point's


def _one(faces, depths, opacities, layers, point=-1, zn=0.0, bias=0.0, group=None):
    """a single sample under G layers"""
    G = len(faces)
    c, d, a, i = scene_layers_ref.compose(np.array(faces).reshape(G, 1), M[:G].reshape(G, 1, 3), np.array(depths, F32).reshape(G, 1),
                                          None if opacities is None else np.array(opacities, F32).reshape(G, 1), layers,
                                          np.array([point]), P[None], np.array([zn], F32), bias, BG, FAR, group)
    assert c.dtype == F32 and d.dtype == F32 and a.dtype == F32 and i.dtype == np.int32
    return c[0], d[0], a[0], i[0]


def _over(o, top, under):
    """o * top + (1 - o) * under: two products, one sum, each rounded once"""
    o = F32(o)
    return ((o * np.asarray(top, F32)).astype(F32) + ((F32(1) - o) * np.asarray(under, F32)).astype(F32)).astype(F32)


@pytest.mark.parametrize("layers", [1, 4])
def test_one_group_is_scene_ref(layers):
    """with a single face layer (any K: there is nothing to list beyond it) the reference equals scene_ref.compose"""
    rs = np.random.RandomState(3)
    n = 4000
    fid = np.where(rs.rand(n) < 0.7, rs.randint(0, 50, n), -1)
    pid = np.where(rs.rand(n) < 0.6, rs.randint(0, 50, n), -1)
    m, p = rs.rand(n, 3).astype(F32), rs.rand(n, 3).astype(F32)
    zf = np.where(fid >= 0, rs.randint(1, 9, n) / F32(4), F32(FAR)).astype(F32)            # a coarse grid: plenty of exact ties
    zn = np.where(pid >= 0, rs.randint(1, 9, n) / F32(4), F32(FAR)).astype(F32)
    op = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0, np.nan], F32), n)
    for opacity in (None, op):
        for bias in (0.0, 0.25):
            want = scene_ref.compose(fid, m, zf, pid, p, zn, opacity, bias, BG, FAR)
            got = scene_layers_ref.compose(fid[None], m[None], zf[None], None if opacity is None else opacity[None], layers, pid, p,
                                           zn, bias, BG, FAR)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w)
    assert ((fid >= 0) & (pid >= 0) & (zf == zn)).sum() > 50


def test_an_opaque_face_cuts_the_list():
    # translucent 0.5 over opaque over a third face that no longer exists, over the background
    c, d, a, i = _one([5, 6, 7], [1.0, 2.0, 3.0], [0.5, 1.0, 0.5], 4)
    assert np.array_equal(c, _over(0.5, M[0], M[1])) and d == F32(1.0) and a == 1 and i == 5
    # the same without the opaque face: the third face shows, and the background through both
    c, d, a, i = _one([5, 6, 7], [1.0, 2.0, 3.0], [0.5, 0.25, 0.5], 4)
    want = _over(0.5, M[0], _over(0.25, M[1], _over(0.5, M[2], BG)))
    assert np.array_equal(c, want) and d == F32(1.0) and i == 5
    # an opaque FIRST face is all there is
    c, d, a, i = _one([5, 6], [1.0, 2.0], [1.0, 0.5], 4)
    assert np.array_equal(c, M[0]) and a == 1 and i == 5
    c, d, a, i = _one([5, 6], [1.0, 2.0], None, 4)                     # no opacities: every face opaque
    assert np.array_equal(c, M[0]) and a == 1 and i == 5


def test_a_point_between_two_faces():
    # the faces behind the point do not exist; the point is what lies under the first
    c, d, a, i = _one([5, 6], [1.0, 3.0], [0.5, 0.5], 4, point=9, zn=2.0)
    assert np.array_equal(c, _over(0.5, M[0], P)) and d == F32(1.0) and a == 1 and i == 5
    # a point in front of both
    c, d, a, i = _one([5, 6], [1.0, 3.0], [0.5, 0.5], 4, point=9, zn=0.5)
    assert np.array_equal(c, P) and d == F32(0.5) and a == 1 and i == -11
    # behind both: under the second
    c, d, a, i = _one([5, 6], [1.0, 3.0], [0.5, 0.5], 4, point=9, zn=3.5)
    assert np.array_equal(c, _over(0.5, M[0], _over(0.5, M[1], P))) and d == F32(1.0) and a == 1 and i == 5
    # equality goes to the face, a bias gives it to the point
    assert np.array_equal(_one([5, 6], [1.0, 3.0], [0.5, 0.5], 4, point=9, zn=3.0)[0], _over(0.5, M[0], _over(0.5, M[1], P)))
    assert np.array_equal(_one([5, 6], [1.0, 3.0], [0.5, 0.5], 4, point=9, zn=3.0, bias=0.01)[0], _over(0.5, M[0], P))
    # behind an opaque face the point does not show, and alpha is 1 either way
    c, d, a, i = _one([5, 6], [1.0, 3.0], [0.5, 1.0], 4, point=9, zn=3.5)
    assert np.array_equal(c, _over(0.5, M[0], M[1])) and a == 1 and i == 5


def test_truncation_at_K():
    faces, depths, ops = [5, 6, 7, 8], [4.0, 1.0, 3.0, 2.0], [0.5, 0.5, 0.5, 0.5]           # by depth: 6, 8, 7, 5
    chain = [M[1], M[3], M[2], M[0]]
    for K in (1, 2, 3, 4, 8):
        want = BG
        for top in reversed(chain[:K]):
            want = _over(0.5, top, want)
        c, d, a, i = _one(faces, depths, ops, K)
        assert np.array_equal(c, want) and d == F32(1.0) and i == 6, K
    # a face of opacity 0 still takes a layer: with K = 2 the third face is not seen through two invisible ones
    c, d, a, i = _one([5, 6, 7], [1.0, 2.0, 3.0], [0.0, 0.0, 1.0], 2)
    assert np.array_equal(c, BG) and a == 0 and d == F32(1.0) and i == 5
    c, d, a, i = _one([5, 6, 7], [1.0, 2.0, 3.0], [0.0, 0.0, 1.0], 3)
    assert np.array_equal(c, M[2]) and a == 1 and d == F32(1.0) and i == 5


def test_only_the_nearest_face_of_a_group_counts():
    # layers 0 and 2 are one group: the far one (a closed mesh's back side) is no layer, so K = 2 reaches the other group
    args = ([5, 6, 7], [1.0, 3.0, 2.0], [0.5, 0.5, 0.5])
    c, d, a, i = _one(*args, 2, group=[4, 9, 4])
    assert np.array_equal(c, _over(0.5, M[0], _over(0.5, M[1], BG))) and i == 5
    c, d, a, i = _one(*args, 2)                                           # ungrouped: the back side takes the second layer
    assert np.array_equal(c, _over(0.5, M[0], _over(0.5, M[2], BG))) and i == 5
    # the ids are labels: any int32 does
    assert np.array_equal(_one(*args, 2, group=[-7, 2 ** 31 - 1, -7])[0], _one(*args, 2, group=[4, 9, 4])[0])
    # K = 1 with groups is the plain rule
    assert np.array_equal(_one(*args, 1, group=[4, 9, 4])[0], _over(0.5, M[0], BG))


def test_a_tie_is_decided_by_the_index():
    z = F32(1.2345678)
    c, d, a, i = _one([8, 3], [z, z], [0.5, 1.0], 4)
    assert np.array_equal(c, M[1]) and i == 3 and a == 1                  # face 3 is first, and opaque
    c, d, a, i = _one([8, 3], [z, z], [1.0, 0.5], 4)
    assert np.array_equal(c, _over(0.5, M[1], M[0])) and i == 3
    c, d, a, i = _one([8, 3], [z, z], [1.0, 0.5], 1)                      # and the one that survives K = 1
    assert np.array_equal(c, _over(0.5, M[1], BG)) and i == 3 and a == F32(0.5)
    # inside a group too: the smaller index is the group's face
    c, d, a, i = _one([8, 3], [z, z], [1.0, 0.5], 4, group=[1, 1])
    assert np.array_equal(c, _over(0.5, M[1], BG)) and i == 3


def test_the_alpha_fold():
    c, d, a, i = _one([5, 6], [1.0, 2.0], [0.5, 0.25], 4)
    assert a == F32(F32(0.5) + F32(0.5) * F32(F32(0.25) + F32(0.75) * F32(0))) and a == F32(0.625)
    assert _one([5], [1.0], [0.3], 4)[2] == F32(0.3)                       # o + (1 - o) * 0 = o: the plain rule's alpha
    assert _one([5, 6], [1.0, 2.0], [0.5, 1.0], 4)[2] == 1                 # an opaque face closes the sample
    assert _one([5, 6], [1.0, 2.0], [0.0, float("nan")], 4)[2] == 0        # NaN -> 0
    assert _one([5, 6], [1.0, 2.0], [0.5, 0.25], 4, point=0, zn=9.0)[2] == 1
    c, d, a, i = _one([-1, -1], [FAR, FAR], [0.5, 0.5], 4)                # nothing at all
    assert np.array_equal(c, BG) and d == F32(FAR) and a == 0 and i == -1


def test_mesh_face_group():
    import torch
    from chore_amd.utils.render_utils import Mesh, mesh_face_group, mesh_face_opacity, mesh_tensors
    tri = Mesh(v=np.eye(3), f=np.array([[0, 1, 2]]))
    quad = Mesh(v=np.zeros((4, 3)), f=np.array([[0, 1, 2], [0, 2, 3]]))
    colours = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    g = mesh_face_group([tri, quad, tri], "cpu", colours)
    assert g.dtype == torch.int32 and g.shape == (1, 4) and g[0].tolist() == [0, 1, 1, 2]
    assert g.shape[1] == mesh_tensors([tri, quad, tri], colours, "cpu")[1].shape[1] == mesh_face_opacity([tri, quad, tri], 0.5, "cpu").shape[1]
    assert mesh_face_group([quad], "cpu")[0].tolist() == [0, 0]
    with pytest.raises(ValueError):
        mesh_face_group([tri, quad, tri], "cpu", colours[:2])             # mesh_tensors would leave the third mesh out


def test_the_new_keywords_come_last():
    from chore_amd.render import Renderer, rasterize_scene
    from chore_amd.utils.render_utils import NrWrapper, render_scene_views
    old = {
        rasterize_scene: ["faces", "textures", "light", "points_ndc", "colors", "radius", "face_opacity", "point_depth_bias",
                          "image_size", "anti_aliasing", "near", "far", "eps", "ambient", "background_color", "return_index"],
        Renderer.render_scene: ["self", "vertices", "faces", "textures", "points", "colors", "radius", "world_radius", "face_opacity",
                                "point_depth_bias", "K", "R", "t", "dist_coeffs", "orig_size"],
        NrWrapper.render_scene: ["self", "renderer", "meshes", "clouds", "colors", "world_radius", "mesh_colors", "mesh_opacity",
                                 "point_depth_bias"],
        render_scene_views: ["images_b", "crop_center_b", "meshes", "mesh_colors", "mesh_opacity", "clouds", "colors", "radii",
                             "markers2d", "point_depth_bias", "side_renderer", "camera", "maxd", "min_radius_px"],
    }
    for fn, names in old.items():
        par = inspect.signature(fn).parameters
        new = ["face_layers", "face_group"] if fn in (rasterize_scene, Renderer.render_scene) else ["face_layers"]
        assert list(par) == names + new, fn.__qualname__
        assert par["face_layers"].default == 1
        assert "face_group" not in par or par["face_group"].default is None
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    assert ReconFitterBase.VIEW_FACE_LAYERS == 1
