"""CPU: the yardstick of the signed mesh-distance tests pins itself (tests/mesh_sign_ref.py), and the host-side parts of the
penetration report: is_closed, the REPORT_PENETRATION default."""
import numpy as np

import mesh_dist_ref
import mesh_sign_ref as sref
from chore_amd.recon.eval.penetration import is_closed
from meshes import icosphere

BOX = ((-0.3, -0.2, 2.0), (0.4, 0.5, 2.6))


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def box_points():
    return f32(np.random.RandomState(1).rand(2400, 3) * 1.6 + np.array([-0.8, -0.7, 1.5]))


def test_oriented_box_against_the_closed_form():
    P = box_points()
    lo, hi = f32(BOX[0]), f32(BOX[1])
    inside = ((P > lo) & (P < hi)).all(1)
    assert inside.sum() > 100 and (~inside).sum() > 1000
    for n in (1, 12):
        V, F = sref.oriented_box(BOX[0], BOX[1], n)
        assert F.shape == (12 * n * n, 3)
        w = sref.winding(P, f32(V), F)
        assert np.array_equal(np.abs(w) > 0.5, inside)
        assert np.abs(w - inside).max() <= 1e-12
    # the box as mesh_dist_ref builds it has half of its faces pointing inward: no integers there
    V, F = mesh_dist_ref.box_mesh(BOX[0], BOX[1], 1)
    assert np.abs(sref.winding(P, f32(V), F) - inside).max() > 0.1


def test_integer_winding_numbers_on_closed_meshes():
    from chore_amd.utils.synth import uv_ellipsoid
    rs = np.random.RandomState(3)
    for name, (V, F) in (("icosphere", icosphere(2, 0.35, (0.45, 0.1, 2.3))), ("uv_ellipsoid", uv_ellipsoid(center=(0.1, 0.2, 2.2)))):
        V = f32(V)
        P = f32(np.concatenate([V.mean(0) + 0.05 * rs.standard_normal((40, 3)), V.mean(0) + 3.0 + rs.rand(40, 3)]))
        w = sref.winding(P, V, F)
        want = np.concatenate([np.ones(40), np.zeros(40)])
        print(name, "max |w - integer| %.3e" % np.abs(w - want).max())
        assert np.abs(w - want).max() <= 1e-12, name
        assert np.abs(sref.winding(P, V, F[:, ::-1]) + want).max() <= 1e-12, name       # inward faces: -1


def test_float32_restatement_and_degenerate_faces():
    V, F = icosphere(2, 0.35, (0.45, 0.1, 2.3))
    V = f32(V)
    P, _ = mesh_dist_ref.sampler_points([(V, F)], 170, 30, np.random.RandomState(0))
    w64, w32 = sref.winding(P, V, F), sref.winding(P, V, F, np.float32)
    assert w32.dtype == np.float32 and 0 < np.abs(w32 - w64).max() < 1e-5
    rs = np.random.RandomState(4)
    i, j = rs.randint(0, len(V), 100), rs.randint(0, len(V), 100)
    deg = np.concatenate([np.zeros((100, 3), np.int64), np.stack([i, i, j], 1)])
    onv = np.concatenate([P[:5], V[:7], V[F[:5]].mean(1)])                    # points on vertices and on face centres too
    for dt in (np.float64, np.float32):
        h = sref.half_angles(onv, V, deg, dt)
        assert (h == 0).all()                                                 # exactly 0, never NaN
        assert np.isfinite(sref.winding(onv, V, np.concatenate([F, deg]), dt)).all()
    assert np.array_equal(sref.winding(P, V, np.concatenate([F, deg]), np.float32), w32)     # added one after the other: same bits
    assert np.abs(sref.winding(P, V, np.concatenate([F, deg])) - w64).max() <= 1e-15
    # a point on a corner of a proper triangle: that triangle contributes exactly 0
    assert (sref.half_angles(V[F[:9, 1]], V, F[:9], np.float32)[np.arange(9), np.arange(9)] == 0).all()


def test_is_closed():
    from chore_amd.recon.assets import SyntheticAssets
    from chore_amd.utils.synth import uv_ellipsoid
    _, Fb = sref.oriented_box(BOX[0], BOX[1], 1)
    _, Fh = sref.hemisphere(2)
    _, Fi = icosphere(2)
    assert Fh.shape == (152, 3)
    assert is_closed(Fi) and is_closed(Fi[:, ::-1]) and is_closed(uv_ellipsoid()[1]) and is_closed(SyntheticAssets(0).template("x")[1])
    assert not is_closed(Fh) and not is_closed(Fi[:-1])
    flipped = Fi.copy()
    flipped[0] = flipped[0, ::-1]
    assert not is_closed(flipped)                                             # every edge twice, one pair in the same direction
    assert not is_closed(np.concatenate([Fi, [[0, 0, 1]]]))
    assert is_closed(Fb) and is_closed(sref.oriented_box(BOX[0], BOX[1], 12)[1])
    assert not is_closed(mesh_dist_ref.box_mesh(BOX[0], BOX[1], 1)[1])        # every side has vertices of its own there
    cube = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6],
                     [3, 0, 4], [3, 4, 7]])
    assert is_closed(cube)
    import torch
    assert is_closed(torch.as_tensor(cube))
    for F in (Fb, Fh, Fi, flipped, cube, Fi[:-1]):
        assert is_closed(F) == sref.is_closed_ref(F)


def test_report_penetration_is_off_by_default():
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    from chore_amd.recon.recon_fit_behave import ReconFitterBehave
    assert ReconFitterBase.REPORT_PENETRATION is False and ReconFitterBehave.REPORT_PENETRATION is False
