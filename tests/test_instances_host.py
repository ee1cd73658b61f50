"""CPU: the yardstick of the instance-mask tests pins itself (tests/instances_ref.py), and the host-side parts of the feature: the
size rule of the C entry point, the argument checks of the Python wrappers, the frame rows of render_masks, the schema of
k*.occlusion.json and the drop-in alias."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import instances_ref as iref
import render_ref
from conftest import REPO
from meshes import icosphere
from oracle import silhouette as osil


def random_tri(seed=0, B=3, V=30, Fn=40):
    """random_tri of tests/test_gpu_render.py"""
    rs = np.random.RandomState(seed)
    v = np.concatenate([rs.uniform(-1.2, 1.2, (B, V, 2)), rs.uniform(0.5, 4.0, (B, V, 1))], -1).astype(np.float32)
    f = np.stack([np.stack([rs.choice(V, 3, replace=False) for _ in range(Fn)]) for _ in range(B)]).astype(np.int64)
    v[1, :, :2] *= 0.3
    v[2, :5] = 0.0
    return osil.vertices_to_faces(v, osil.fill_back(f))


def test_restatement_invariants():
    tri = random_tri(0)
    grp = np.broadcast_to(np.asarray([(0, 1, 2, -1, 3)[(f % 40) % 5] for f in range(80)]), (3, 80))
    for size, ssaa in ((33, 1), (32, 2)):
        ref = iref.instances(tri, grp, 3, size, ssaa)
        vis, cov = ref["vis"], ref["cov"]
        assert vis.sum(1).max() == 1 and (vis <= cov).all() and (vis < cov).any()
        assert ref["visible"].shape == (3, 3, size, size) and ref["visible"].dtype == np.float32
        assert (ref["visible"].sum(1) <= 1).all() and (ref["visible"] <= ref["full"]).all()
        n = ssaa * ssaa
        assert np.array_equal(ref["visible"].sum((2, 3)) * n, ref["group_samples"][..., 0])
        assert np.array_equal(ref["full"].sum((2, 3)) * n, ref["group_samples"][..., 1])
        assert np.array_equal(np.unique(ref["full"] * n), np.arange(n + 1))
        # the occluders (groups -1 and 3 at G = 3) win samples that no group counts
        won = (ref["face_index"] >= 0).sum((1, 2))
        assert np.array_equal(ref["face_samples"].sum(1), won) and (ref["group_samples"][..., 0].sum(1) < won).all()
        # the flip: sample row block y lands in image row size - 1 - y
        top = vis[:, :, :ssaa].any(2).reshape(3, 3, size, ssaa).any(3)
        assert np.array_equal(ref["visible"][:, :, -1] > 0, top)
    none = iref.instances(tri, None, 1, 32, 2)
    assert np.array_equal(none["visible"], none["full"])
    assert np.array_equal(none["visible"][:, 0], render_ref.resolve(np.zeros((3, 64, 64, 3), np.float32), np.zeros((3, 64, 64), np.float32),
                                                                    (none["face_index"] >= 0).astype(np.float32), 2)[2])


def test_boxed_winners_are_the_winners():
    """winners_boxed (used where a mesh has too many faces for the full-image restatement) against render_ref.winners"""
    tri = random_tri(0)
    for S in (61, 128):
        assert np.array_equal(iref.winners_boxed(tri, S), render_ref.winners(tri, S))
    v, f = icosphere(2, 0.5, (0.1, 0.2, 2.0))
    tri = osil.vertices_to_faces((v / v[:, 2:] * [1.0, 1.0, 0.0] + [0, 0, 1] * v[:, 2:]).astype(np.float32)[None], osil.fill_back(f[None]))
    fim = render_ref.winners(tri, 96)
    assert 0.05 < (fim >= 0).mean() < 0.5 and np.array_equal(iref.winners_boxed(tri, 96), fim)


def test_instances_workspace_bytes():
    from chore_amd import _lib
    ws, render_ws = _lib.lib.chore_instances_workspace_bytes, _lib.lib.chore_render_workspace_bytes
    for B, Fn, size, ssaa in ((1, 1000, 256, 2), (3, 80, 61, 1), (2, 30112, 2048, 2)):
        for G in (1, 2, 8):
            assert ws(B, Fn, G, size, ssaa) == render_ws(B, Fn, size, ssaa) > 0
    assert ws(1, 80, 0, 64, 2) == 0 and ws(1, 80, 9, 64, 2) == 0 and ws(1, 80, -1, 64, 2) == 0
    assert ws(1, 80, 1, 64, 3) == 0 and ws(1, 80, 1, 64, 0) == 0
    assert ws(1, 80, 1, 2049, 2) == 0 and ws(1, 80, 1, 4096, 1) > 0 and ws(1, 80, 1, 4097, 1) == 0
    assert ws(0, 80, 1, 64, 2) == 0 and ws(1, 0, 1, 64, 2) == 0


def test_wrappers_need_device_tensors():
    """no CPU path: RuntimeError on CPU tensors from every entry of the feature, before any argument is looked at"""
    from chore_amd import render as nr
    from chore_amd.preprocess import render_masks
    from chore_amd.recon.eval.occlusion import occlusion
    from chore_amd.utils.render_utils import Mesh, setup_renderer
    assert nr.face_visibility is nr.renderer.face_visibility and nr.rasterize_instances is nr.renderer.rasterize_instances
    tri = torch.from_numpy(random_tri(0))
    with pytest.raises(RuntimeError):
        nr.rasterize_instances(tri, None, 1, 64)
    with pytest.raises(RuntimeError):
        nr.rasterize_instances(tri, None, 0, 64)
    with pytest.raises(RuntimeError):
        nr.face_visibility(tri, 64)
    v, f = icosphere(1, 0.3, (0.0, 0.0, 2.2))
    vt, ft = torch.as_tensor(v, dtype=torch.float32)[None], torch.as_tensor(f)[None]
    for r in (setup_renderer(image_size=64), nr.Renderer(camera_mode="look_at", image_size=64)):
        with pytest.raises(RuntimeError):
            r.visibility(vt, ft)
        with pytest.raises(RuntimeError):
            r(vt, ft, mode="visibility")
        with pytest.raises(RuntimeError):
            r.render_instances(vt, ft, torch.zeros(1, len(f), dtype=torch.int32), 1)
        with pytest.raises(ValueError):
            r(vt, ft, mode="normals")
    with pytest.raises(RuntimeError):
        occlusion(vt, ft[0], vt, ft[0], image_size=64)
    with pytest.raises(RuntimeError):
        render_masks(Mesh(v=v, f=f), Mesh(v=v, f=f), image_size=64, device="cpu")


def test_frame_rows():
    from chore_amd.preprocess import frame_rows
    assert frame_rows(2048) == 1536 and frame_rows(1024) == 768 and frame_rows(256) == 192 and frame_rows(64) == 48
    assert frame_rows(250) == 187 and frame_rows(1) == 0                  # rounded down: a row that is only partly the frame's is left out
    assert frame_rows(100, 1080, 1920) == 56 and frame_rows(512, 512, 512) == 512
    for bad in ((0, 1536, 2048), (256, 0, 2048), (256, 1536, 0), (256, 2048, 1536)):
        with pytest.raises(ValueError):
            frame_rows(*bad)


def test_occlusion_json_schema():
    from chore_amd.recon.eval.occlusion import COUNT_KEYS, MIN_VISIBLE, frame_report
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    from chore_amd.recon.recon_fit_behave import ReconFitterBehave
    assert MIN_VISIBLE == 0.30 and COUNT_KEYS == ("body_visible", "body_full", "object_visible", "object_full")
    assert ReconFitterBase.REPORT_OCCLUSION is False and ReconFitterBehave.REPORT_OCCLUSION is False
    rep = frame_report(np.int64(901), 2047, torch.tensor(1930), 1930)
    assert rep == {"body_visible": 901, "body_full": 2047, "object_visible": 1930, "object_full": 1930,
                   "body_fraction": 901 / 2047, "object_fraction": 1.0, "object_evaluated": True}
    assert json.loads(json.dumps(rep)) == rep and all(type(rep[k]) is int for k in COUNT_KEYS)
    # the reference skips a frame when visible / full < 0.30 (evaluate.py:57): 0.30 itself is evaluated
    assert frame_report(5, 5, 3, 10)["object_evaluated"] is True and frame_report(5, 5, 300, 1000)["object_evaluated"] is True
    assert frame_report(5, 5, 299, 1000)["object_evaluated"] is False and frame_report(5, 5, 0, 7)["object_evaluated"] is False
    gone = frame_report(5, 5, 0, 0)
    assert gone["object_fraction"] is None and gone["object_evaluated"] is False and gone["body_fraction"] == 1.0
    assert "NaN" not in json.dumps(gone) and frame_report(0, 0, 1, 1)["body_fraction"] is None


def test_dropin_face_visibility_alias(tmp_path):
    """`import neural_renderer as nr; nr.face_visibility` resolves inside a CHORE checkout after dropin.install (the stand-in
    checkout of tests/test_render_host.py)"""
    root = tmp_path / "chore"
    root.mkdir()
    (root / "PATHS.yml").write_text('RECON_PATH: "recon_out"\nSMPL_ASSETS_ROOT: "assets"\n')
    for pkg in ("config", "recon", "utils"):
        (root / pkg).mkdir()
    (root / "config" / "__init__.py").write_text("")
    (root / "config" / "config_loader.py").write_text('"""stand-in for the checkout\'s config loader"""\n')
    (root / "utils" / "__init__.py").write_text("")
    code = ("import chore_amd.dropin as d; d.install(); import neural_renderer as nr; "
            "from neural_renderer.renderer import Renderer; "
            "assert callable(nr.face_visibility) and callable(nr.rasterize_instances) and callable(Renderer.visibility); "
            "print(nr.face_visibility.__module__)")
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run([sys.executable, "-c", code], cwd=str(root), capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-1] == "chore_amd.render.renderer"
