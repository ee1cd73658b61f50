"""CPU: the yardstick of the mesh-distance tests against known answers, the host logic of BoundarySampler and
BodyLandmarks, and the drop-in aliases of the preprocessing modules."""
import os
import pickle
import subprocess
import sys

import numpy as np

import mesh_dist_ref as ref
from conftest import GOLDEN, REPO

ASSETS = os.path.join(GOLDEN, "assets")


# ---- 1. the yardstick itself -----------------------------------------------------------------------------------------
def test_ref_box_against_closed_form():
    lo, hi = (-0.3, -0.2, 2.0), (0.4, 0.5, 2.6)
    V, F = ref.box_mesh(lo, hi, 12)
    assert F.shape == (1728, 3)
    rs = np.random.RandomState(1)
    P = rs.rand(2000, 3) * 1.6 + np.array([-0.8, -0.7, 1.5])
    inside = ((P > lo) & (P < hi)).all(1)
    assert inside.sum() > 100 and (~inside).sum() > 1000
    D, I, C = ref.mesh_distance_pruned(P, V, F)
    want = ref.box_distance(P, lo, hi)
    print("box: max |restatement - closed form| = %.3e" % np.abs(D - want).max())
    assert np.abs(D - want).max() <= 1e-12
    assert np.abs(np.linalg.norm(P - C, axis=1) - D).max() <= 1e-12
    Db, _, _ = ref.mesh_distance_brute(P[:300], V, F)
    assert np.abs(Db - want[:300]).max() <= 1e-12


def test_ref_one_triangle_seven_regions():
    a, b, c = np.array([0.0, 0, 0]), np.array([2.0, 0, 0]), np.array([0.0, 2, 0])
    V, F = np.stack([a, b, c]), np.array([[0, 1, 2]])
    s = 2 ** 0.5
    cases = [  # point, closest point
        ((0.5, 0.5, 0.7), (0.5, 0.5, 0.0)),         # interior
        ((-1.0, -1.0, 0.5), (0.0, 0.0, 0.0)),       # vertex a
        ((3.0, -0.5, 0.0), (2.0, 0.0, 0.0)),        # vertex b
        ((-0.5, 3.0, 1.0), (0.0, 2.0, 0.0)),        # vertex c
        ((1.0, -2.0, 0.0), (1.0, 0.0, 0.0)),        # edge ab
        ((-2.0, 1.0, 1.0), (0.0, 1.0, 0.0)),        # edge ac
        ((2.0, 2.0, 0.0), (1.0, 1.0, 0.0)),         # edge bc
    ]
    P = np.array([p for p, _ in cases])
    Q = np.array([q for _, q in cases])
    for fn in (ref.mesh_distance_brute, ref.mesh_distance_pruned):
        D, I, C = fn(P, V, F)
        assert np.abs(C - Q).max() <= 1e-14 and np.abs(D - np.linalg.norm(P - Q, axis=1)).max() <= 1e-14
        assert np.all(I == 0)
    assert abs(ref.mesh_distance_brute(P[6:7], V, F)[0][0] - s) <= 1e-15


def test_ref_pruned_equals_brute_bit_for_bit():
    from meshes import icosphere
    from chore_amd.utils.synth import uv_ellipsoid
    body = uv_ellipsoid(center=(0.1, 0.2, 2.2))
    obj = icosphere(3, 0.35, (0.45, 0.1, 2.3))
    P, tag = ref.sampler_points([body, obj], 150, 17, np.random.RandomState(2))
    P = P[np.random.RandomState(3).permutation(len(P))[:500]]
    assert len(P) == 500
    for V, F in (body, obj):
        Db, Ib, Cb = ref.mesh_distance_brute(P, V, F)
        Dp, Ip, Cp = ref.mesh_distance_pruned(P, V, F)
        assert np.array_equal(Db, Dp) and np.array_equal(Ib, Ip) and np.array_equal(Cb, Cp)


def test_ref_degenerate_triangles():
    V = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 2, 0]], np.float64)
    P = np.array([[0.5, 1, 0], [3, 0, 1], [-1, -1, 0], [1.0, 1.0, 0.5]])

    def seg(p, a, b):
        t = np.clip(((p - a) @ (b - a)) / max((b - a) @ (b - a), 1e-300), 0, 1)
        return np.linalg.norm(p - (a + t[:, None] * (b - a)), axis=1)
    cases = [([0, 1, 2], seg(P, V[0], V[2])), ([0, 2, 1], seg(P, V[0], V[2])),        # collinear: the segment 0-2
             ([0, 0, 3], seg(P, V[0], V[3])), ([0, 3, 3], seg(P, V[0], V[3])), ([3, 0, 0], seg(P, V[0], V[3])),  # repeated vertex
             ([1, 1, 1], np.linalg.norm(P - V[1], axis=1))]                            # a point
    for f, want in cases:
        for dt in (np.float64, np.float32):
            D, _, C = ref.mesh_distance_brute(P, V, np.array([f]), dt)
            assert np.isfinite(D).all() and np.isfinite(C).all()
            assert np.abs(D - want).max() <= (1e-14 if dt is np.float64 else 1e-6), (f, dt, D, want)


# ---- 2. BoundarySampler host logic -----------------------------------------------------------------------------------
def test_boundary_sampler_host_logic():
    from chore_amd.preprocess.boundary_sampler import BoundarySampler
    s = BoundarySampler()
    assert s.get_sample_num(0.01, 100000) == 10000 and s.get_sample_num(0.49, 100000) == 49000
    assert s.get_sample_num(0.5, 100000) == 50000 and s.get_sample_num(0.5, 1000) == 10000
    assert s.get_sample_num(0.5, 1000, thres=100) == 500
    parts = np.arange(14).astype(np.int32)
    flipped = s.flip_part_labels(parts)
    want = parts.copy()
    for l, r in ((1, 6), (2, 7), (3, 8), (4, 9), (5, 10), (12, 13)):
        want[l], want[r] = r, l
    assert np.array_equal(flipped, want) and flipped.dtype == parts.dtype
    assert np.array_equal(parts, np.arange(14)) and np.array_equal(s.flip_part_labels(flipped), parts)
    assert [k for k in range(14) if flipped[k] == k] == [0, 11]
    big = np.random.RandomState(0).randint(0, 14, 1000).astype(np.uint8)
    assert np.array_equal(s.flip_part_labels(big), want[big])
    bmin, bmax = BoundarySampler.get_bounds()
    assert np.array_equal(bmin, [-3.0, -0.9, 0.2]) and np.array_equal(bmax, [3.0, 1.8, 4.0])


def test_boundary_sampler_label_table(tmp_path, monkeypatch):
    from chore_amd.preprocess.boundary_sampler import BoundarySampler
    part_labels = pickle.load(open(os.path.join(ASSETS, "smpl_parts_dense.pkl"), "rb"))
    labels = np.zeros((6890,), dtype="int32")
    for n, k in enumerate(part_labels):
        labels[part_labels[k]] = n
    assert len(part_labels) == 14 and set(np.unique(labels)) == set(range(14))
    # default: ./assets/smpl_parts_dense.pkl, like the reference
    os.symlink(ASSETS, tmp_path / "assets")
    monkeypatch.chdir(tmp_path)
    got = BoundarySampler().part_labels
    assert got.dtype == np.int32 and np.array_equal(got, labels)
    # or PATHS.yml's SMPL_ASSETS_ROOT
    other = tmp_path / "elsewhere"
    other.mkdir()
    (other / "PATHS.yml").write_text('SMPL_ASSETS_ROOT: "%s"\n' % ASSETS)
    monkeypatch.chdir(other)
    assert np.array_equal(BoundarySampler().part_labels, labels)
    given = BoundarySampler(part_labels=labels[::-1].copy(), seed=3, device="cuda:0")
    assert np.array_equal(given.part_labels, labels[::-1])


# ---- 3. BodyLandmarks ------------------------------------------------------------------------------------------------
class _Mesh:
    def __init__(self, v):
        self.v = v


def test_body_landmarks():
    from chore_amd.lib_smpl.body_landmark import BodyLandmarks
    lm = BodyLandmarks(ASSETS)
    v = np.random.RandomState(4).standard_normal((6890, 3))
    reg = pickle.load(open(os.path.join(ASSETS, "body25_regressor.pkl"), "rb"), encoding="latin1").T
    want = reg.dot(v)
    assert want.shape == (25, 3)
    kpts = lm.get_body_kpts(_Mesh(v))
    assert np.array_equal(np.asarray(kpts), np.asarray(want))
    assert np.array_equal(np.asarray(lm.get_smpl_center(_Mesh(v))), np.asarray(want)[8])
    body, face, hand = lm.get_landmarks(_Mesh(v))
    assert np.array_equal(np.asarray(body), np.asarray(want)) and face.shape == (70, 3) and hand.shape == (42, 3)
    parts = lm.load_parts_ind(os.path.join(ASSETS, "smpl_parts_dense.pkl"))
    name = next(iter(parts))
    pv = lm.get_part_verts(v, name)
    assert np.array_equal(pv, v[parts[name]]) and not np.shares_memory(pv, v)

    class Tri:      # a trimesh-style mesh
        vertices = v
    assert np.array_equal(np.asarray(lm.get_body_kpts(Tri())), np.asarray(want))


# ---- 4. drop-in ------------------------------------------------------------------------------------------------------
def test_dropin_preprocess_aliases(tmp_path):
    """inside a CHORE checkout `preprocess.boundary_sampler` and `lib_smpl.body_landmark` are this package's, while
    preprocess/preprocess_scale.py (the driver) is still the checkout's file"""
    root = tmp_path / "chore"
    root.mkdir()
    (root / "PATHS.yml").write_text('RECON_PATH: "recon_out"\nSMPL_ASSETS_ROOT: "assets"\n')
    (root / "config").mkdir()
    (root / "config" / "__init__.py").write_text("")
    (root / "config" / "config_loader.py").write_text('"""stand-in for the checkout\'s config loader"""\n')
    (root / "preprocess").mkdir()
    (root / "preprocess" / "preprocess_scale.py").write_text('"""stand-in for the checkout\'s driver"""\nMARK = "checkout"\n')
    (root / "preprocess" / "boundary_sampler.py").write_text('raise ImportError("the checkout\'s sampler must not be imported")\n')
    (root / "lib_smpl").mkdir()
    (root / "lib_smpl" / "body_landmark.py").write_text('raise ImportError("the checkout\'s landmarks must not be imported")\n')
    code = ("import chore_amd.dropin as d; d.install(); "
            "from preprocess.boundary_sampler import BoundarySampler; from lib_smpl.body_landmark import BodyLandmarks; "
            "import preprocess.preprocess_scale as ps; import preprocess; "
            "print(BoundarySampler.__module__, BodyLandmarks.__module__, ps.__file__, ps.MARK, preprocess.__name__)")
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run([sys.executable, "-c", code], cwd=str(root), capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    mods = out.stdout.split()
    assert mods[0] == "chore_amd.preprocess.boundary_sampler" and mods[1] == "chore_amd.lib_smpl.body_landmark"
    assert mods[2].startswith(str(root)) and mods[3] == "checkout" and mods[4] == "chore_amd.preprocess"
