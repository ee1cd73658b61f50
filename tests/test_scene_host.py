"""CPU: the composite rule of tests/scene_ref.py on hand-made layers, and render_utils.icosphere_mesh."""
import numpy as np

import scene_ref

F32 = np.float32
BG = (0.25, 0.5, 0.75)
FAR = 100.0
M = np.array([0.8, 0.4, 0.2], F32)          # the face's colour
P = np.array([0.1, 0.6, 0.9], F32)          # the point's


def _one(face, zf, point, zn, opacity=None, bias=0.0):
    """a single sample: face id / depth, point id / depth"""
    c, d, a, i = scene_ref.compose(np.array([face]), M[None], np.array([zf], F32), np.array([point]), P[None],
                                   np.array([zn], F32), None if opacity is None else np.array([opacity], F32), bias, BG, FAR)
    assert c.dtype == F32 and d.dtype == F32 and a.dtype == F32 and i.dtype == np.int32
    return c[0], d[0], a[0], i[0]


def test_point_in_front():
    c, d, a, i = _one(7, 2.0, 5, 1.5)
    assert np.array_equal(c, P) and d == F32(1.5) and a == 1 and i == -7
    c, d, a, i = _one(-1, FAR, 0, 1.5, opacity=0.0)          # no face at all: the opacity is not looked at
    assert np.array_equal(c, P) and d == F32(1.5) and a == 1 and i == -2


def test_point_behind_an_opaque_face():
    for op in (None, 1.0, 3.0):
        c, d, a, i = _one(7, 1.0, 5, 1.5, opacity=op)
        assert np.array_equal(c, M) and d == F32(1.0) and a == 1 and i == 7


def test_point_behind_a_translucent_face():
    c, d, a, i = _one(7, 1.0, 5, 1.5, opacity=0.5)
    # 0.5 * (0.8, 0.4, 0.2) + 0.5 * (0.1, 0.6, 0.9): halving is exact in float32, the sum is rounded once
    want = np.array([F32(F32(0.4) + F32(0.05)), F32(F32(0.2) + F32(0.3)), F32(F32(0.1) + F32(0.45))], F32)
    assert np.array_equal(c, want) and np.allclose(c, (0.45, 0.5, 0.55), atol=1e-7)
    assert d == F32(1.0) and a == 1 and i == 7               # a point covers the sample: it is opaque as a whole
    c, d, a, i = _one(7, 1.0, -1, 0.0, opacity=0.5)          # nothing behind: over the background, alpha = the opacity
    want = (F32(0.5) * M + F32(0.5) * np.asarray(BG, F32)).astype(F32)
    assert np.array_equal(c, want) and a == F32(0.5) and d == F32(1.0) and i == 7
    c, d, a, i = _one(7, 1.0, 5, 1.5, opacity=float("nan"))   # NaN -> 0: the point shows through untouched
    assert np.array_equal(c, P) and a == 1 and d == F32(1.0) and i == 7
    c, d, a, i = _one(7, 1.0, -1, 0.0, opacity=-2.0)          # clamped to 0: the background, alpha 0, still the face's depth
    assert np.array_equal(c, np.asarray(BG, F32)) and a == 0 and d == F32(1.0) and i == 7


def test_equality_goes_to_the_face():
    z = F32(1.2345678)
    c, d, a, i = _one(3, z, 9, z)
    assert np.array_equal(c, M) and i == 3 and d == z and a == 1
    below = np.nextafter(z, F32(0))
    assert _one(3, z, 9, below)[3] == -11


def test_equality_with_a_bias_goes_to_the_point():
    z = F32(1.2345678)
    c, d, a, i = _one(3, z, 9, z, bias=0.01)
    assert np.array_equal(c, P) and i == -11 and d == z and a == 1
    assert _one(3, z, 9, z + F32(0.02), bias=0.01)[3] == 3           # further behind than the bias reaches
    assert _one(3, z, 9, F32(z + F32(0.01)), bias=0.01)[3] == (-11 if F32(F32(z + F32(0.01)) - F32(0.01)) < z else 3)


def test_empty_sample():
    c, d, a, i = _one(-1, FAR, -1, FAR, opacity=0.5, bias=0.3)
    assert np.array_equal(c, np.asarray(BG, F32)) and d == F32(FAR) and a == 0 and i == -1


def test_resolve_is_the_renderers():
    """the four samples of a pixel are summed row by row from 0 and scaled by 1/4; rows are flipped"""
    rs = np.random.RandomState(0)
    col, dep, alp = rs.rand(2, 4, 4, 3).astype(F32), rs.rand(2, 4, 4).astype(F32), rs.rand(2, 4, 4).astype(F32)
    rgb, depth, alpha = scene_ref.resolve(col, dep, alp, 2)
    assert rgb.shape == (2, 3, 2, 2) and depth.shape == (2, 2, 2)
    want = (((dep[0, 0, 2] + dep[0, 0, 3]) + dep[0, 1, 2]) + dep[0, 1, 3]) * F32(0.25)
    assert depth[0, 1, 1] == want                                   # sample rows 0..1 are output row size - 1
    one = scene_ref.resolve(col, dep, alp, 1)
    assert np.array_equal(one[1], dep[:, ::-1]) and np.array_equal(one[0], col[:, ::-1].transpose(0, 3, 1, 2))


def test_icosphere_mesh():
    from chore_amd.utils.render_utils import icosphere_mesh
    centre = np.array([0.3, -1.2, 2.5])
    for subdiv, nf in ((0, 20), (1, 80), (2, 320)):
        mesh = icosphere_mesh(centre, 0.06, subdiv)
        v, f = np.asarray(mesh.v), np.asarray(mesh.f)
        assert f.shape == (nf, 3) and v.shape == (nf // 2 + 2, 3)
        assert np.allclose(np.linalg.norm(v - centre, axis=1), 0.06, rtol=0, atol=1e-12)
        edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
        assert len(v) - len(edges) + len(f) == 2
        assert sorted(np.unique(f)) == list(range(len(v)))
        # every directed edge once: a closed, consistently wound surface
        directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert len(np.unique(directed, axis=0)) == len(directed) == 2 * len(edges)
        tri = v[f]
        normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert (np.einsum("fk,fk->f", normal, tri.mean(axis=1) - centre) > 0).all()
    assert np.asarray(icosphere_mesh((0, 0, 0), 1.0).f).shape == (320, 3)


def test_mesh_face_opacity_needs_a_colour_and_an_opacity_per_mesh():
    """mesh_tensors leaves a mesh without a colour out, so the opacity must not be built for more meshes than are drawn"""
    import pytest
    from chore_amd.utils.render_utils import Mesh, mesh_face_opacity
    tri = Mesh(v=np.eye(3), f=np.array([[0, 1, 2]]))
    quad = Mesh(v=np.zeros((4, 3)), f=np.array([[0, 1, 2], [0, 2, 3]]))
    op = mesh_face_opacity([tri, quad], [0.25, 1.0], "cpu", colors=[(1, 0, 0), (0, 1, 0)])
    assert op.shape == (1, 3) and op[0].tolist() == [0.25, 1.0, 1.0]
    assert mesh_face_opacity([tri, quad], 0.5, "cpu")[0].tolist() == [0.5, 0.5, 0.5]
    with pytest.raises(ValueError):
        mesh_face_opacity([tri, quad, tri], 0.5, "cpu", colors=[(1, 0, 0), (0, 1, 0)])
    with pytest.raises(ValueError):
        mesh_face_opacity([tri, quad], [0.5], "cpu")
