"""Host: the yardstick of the mesh-distance gradient (tests/mesh_grad_ref.py) checked against central differences, the
tie cap on every case the GPU tests compare on, and the float64 descent of the two-sphere interpenetration case."""
import numpy as np
import pytest

import mesh_grad_ref as gref


@pytest.fixture(scope="module")
def cases():
    return {n: gref.make_case(n) for n in gref.CASES}


@pytest.mark.parametrize("name", ["ico2", "box12"])
def test_restatement_equals_central_differences(cases, name):
    """d/dP and d/dV of sum_i g_i d_i in float64 against central differences with h = 1e-6, 1e-6 absolute; the closest points
    fall on vertices, edges and interiors"""
    c = cases[name]
    r = c["r64"]
    kinds = (r["bary"] > 1e-9).sum(1)
    print("%s: closest points on vertex / edge / interior: %s" % (name, [(kinds == k).sum() for k in (1, 2, 3)]))
    if name == "ico2":
        assert all((kinds == k).sum() > 20 for k in (1, 2, 3))
    eP = np.abs(gref.fd_points(c["P"], c["V"], c["F"], c["g"]) - r["dP"]).max()
    eV = np.abs(gref.fd_verts(c["P"], c["V"], c["F"], c["g"]) - r["dV"]).max()
    print("%s: worst deviation from central differences: points %.2e, vertices %.2e" % (name, eP, eV))
    assert eP <= 1e-6 and eV <= 1e-6
    assert np.abs(r["bary"].sum(1) - 1).max() <= 1e-12 and r["bary"].min() >= 0
    assert np.abs(np.linalg.norm(r["dP"][c["g"] != 0], axis=1) - c["g"][c["g"] != 0]).max() <= 1e-9      # unit normals times g


@pytest.mark.parametrize("name", gref.CASES)
def test_tie_cap_and_e32(cases, name):
    """at most 1 % of a case's points are left out as ties; E32 of dP and of dV lies in (0, 1e-2)"""
    c = cases[name]
    print("%s: %d of %d points are ties; E32 dist %.2e  dP %.2e  dV %.2e;  d >= %.0e (%d points): dP %.2e  dV %.2e"
          % (name, c["tie"].sum(), len(c["P"]), c["E32_dist"], c["E32_dP"], c["E32_dV"], gref.SHARP, (c["g_sharp"] != 0).sum(),
             c["E32_dP_sharp"], c["E32_dV_sharp"]))
    assert c["tie"].sum() <= gref.TIE_CAP * len(c["P"])
    for k in ("E32_dP", "E32_dV", "E32_dP_sharp", "E32_dV_sharp"):
        assert 0 < c[k] < 1e-2, k
    assert (c["g_sharp"] != 0).sum() >= 0.4 * len(c["P"])
    assert c["E32_dP_sharp"] <= c["E32_dP"]


def test_degenerate_faces_get_finite_weights():
    """the barycentric weights of the closest point of a zero-area triangle (a segment, a point): finite, >= 0, sum 1"""
    rs = np.random.RandomState(3)
    a, d = rs.standard_normal((50, 3)), rs.standard_normal((50, 3))
    seg = gref.barycentric(a + 0.3 * d, a, a + d, a + 2 * d)             # three corners on a line
    rep = gref.barycentric(a + 0.3 * d, a, a, a + d)                     # a repeated corner
    pt = gref.barycentric(a + 0.3 * d, a, a, a)                          # a point
    for b in (seg, rep, pt):
        assert np.isfinite(b).all() and b.min() >= 0 and np.abs(b.sum(1) - 1).max() <= 1e-12
    c = a[:, None, :] * 0 + np.stack([a, a + d, a + 2 * d], 1)
    assert np.abs((seg[:, :, None] * c).sum(1) - (a + 0.3 * d)).max() <= 1e-9      # and they reproduce the point on the segment


def test_two_sphere_descent_float64():
    """steps of 0.05 m along the negative normalized gradient of pen(A,B) + pen(B,A), moving the small sphere only: the loss
    strictly decreases and reaches exactly 0 in 7 steps, the gradient points along the centre line"""
    hist = gref.descent()
    loss = [h[0] for h in hist]
    print("loss", ["%.4f" % x for x in loss], "inside", [h[2] for h in hist])
    assert np.allclose(loss, [0.0416, 0.0301, 0.0205, 0.0125, 0.0064, 0.0024, 0.0004, 0.0], atol=5e-5)
    assert all(b < a for a, b in zip(loss, loss[1:])) and loss[-1] == 0 and len(hist) == 8
    assert hist[0][2] == (38, 7) and hist[-1][2] == (0, 0) and not hist[-1][1].any()
    line = np.array([1.13, 0.21, 2.37]) - np.array([0.0, 0.0, 2.2])
    for h in hist[:-1]:
        cur = line + h[3]                                                             # the centre line of this step
        cos = -(h[1] @ cur) / (np.linalg.norm(h[1]) * np.linalg.norm(cur))            # descent moves B away from A
        assert cos >= 0.999, cos
