"""CPU: the host side of the renderer (chore_amd.render, chore_amd.utils.render_utils) against what the reference's own
Python computes (tests/golden/render_host.npz, written by tests/golden/make_render_golden.py), the drop-in aliases of
`utils.render_utils` / `neural_renderer`, and the workspace query of the kernel.

Tolerances come from the fixture: `bound_<name>` is the largest difference between the reference's float32 result and the
same formula in float64; 4 x that is allowed."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import REPO, golden


@pytest.fixture(scope="module")
def g():
    return golden("render_host.npz")


def _meshes(g):
    from chore_amd.utils.render_utils import Mesh
    return [Mesh(v=g["mesh%d_v" % i], f=g["mesh%d_f" % i]) for i in range(2)]


def _wrapper():
    from chore_amd.utils.render_utils import NrWrapper
    return NrWrapper(device="cpu", image_size=64)


def _pattern(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 3 + yy * 5) % 251, (xx * 7 + yy * 2) % 241, (xx + yy * 11) % 239], -1).astype(np.uint8)


def test_fixture_is_small_and_described(g):
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "render_host.npz")) < 200 * 1024
    assert "crop_size == train_crop_size" in str(g["description"])
    assert "literals of the generator" in str(g["description"])     # the light settings are not recorded reference behaviour
    assert g["mesh0_v"].shape[0] >= 50 and g["mesh0_f"].shape[0] >= 80 and g["mesh1_v"].shape[0] >= 50 and g["mesh1_f"].shape[0] >= 80


def test_prepare_render_and_faces_textures(g):
    from chore_amd.utils import render_utils as ru
    assert np.array_equal(np.asarray(ru.SMPL_OBJ_COLOR_LIST), g["colors"])
    verts, faces, textures = _wrapper().prepare_render(_meshes(g))
    F = g["mesh0_f"].shape[0] + g["mesh1_f"].shape[0]
    assert tuple(faces.shape) == (1, F, 3) and tuple(textures.shape) == (1, F, 4, 4, 4, 3)
    assert faces.dtype == torch.int32 and textures.dtype == torch.float32 and verts.dtype == torch.float32
    assert np.array_equal(verts.numpy(), g["comb_verts"])
    assert np.array_equal(faces.numpy(), g["comb_faces"])
    assert np.array_equal(textures.numpy(), g["comb_textures"])
    # the second mesh indexes the concatenated vertices
    assert faces[0, g["mesh0_f"].shape[0]:].min() >= g["mesh0_v"].shape[0]
    f2, t2 = ru.get_faces_and_textures([verts[:, :60], verts[:, 60:]],
                                       [torch.from_numpy(g["mesh0_f"]), torch.from_numpy(g["mesh1_f"])])
    assert np.array_equal(f2.numpy(), g["comb_faces"]) and np.array_equal(t2.numpy(), g["comb_textures"])


@pytest.mark.parametrize("name", ["front", "side"])
def test_lighting(g, name):
    from chore_amd import render as nr
    from chore_amd.utils import render_utils as ru
    tex = torch.from_numpy(g["light_textures"])
    tex2 = torch.cat((tex, tex.permute((0, 1, 4, 3, 2, 5))), dim=1)
    faces2 = torch.cat((torch.from_numpy(g["comb_faces"]), torch.from_numpy(g["comb_faces"]).flip(-1)), dim=1)
    tri = nr.vertices_to_faces(torch.from_numpy(g["comb_verts"]), faces2)
    assert np.array_equal(tri.numpy(), g["tri_world"])
    r = ru.setup_renderer(image_size=64) if name == "front" else ru.setup_side_renderer(2.0, 0., 90.)
    args = (r.light_intensity_ambient, r.light_intensity_directional, r.light_color_ambient, r.light_color_directional,
            r.light_direction)
    assert np.allclose([args[0], args[1]] + list(args[4]), g["light_args_" + name], rtol=0, atol=1e-15)
    keep = tex2.clone()
    lit = nr.lighting(tri, tex2, *args)
    assert torch.equal(tex2, keep)                                  # ours does not modify its input
    bound = 4 * float(g["bound_lit_" + name])
    assert 0 < bound < 1e-5
    assert np.abs(lit.numpy() - g["lit_" + name]).max() <= bound
    light = nr.face_light(tri, *args)
    assert tuple(light.shape) == (1, faces2.shape[1], 3)
    assert np.abs(light.numpy() - g["light64_" + name]).max() <= bound
    assert g["light64_" + name].max() > 0.6                        # the un-normalised direction is kept


def test_look_at_perspective_side_view(g):
    from chore_amd import render as nr
    from chore_amd.utils import render_utils as ru
    eye = nr.get_points_from_angles(2.0, 0., 90.)
    assert np.array_equal(np.asarray(eye, np.float64), g["side_eye"])
    r = ru.setup_side_renderer(2.0, 0., 90.)
    assert r.camera_mode == "look_at" and r.image_size == 640 and tuple(r.eye) == tuple(eye)
    meshes = _meshes(g)
    w = _wrapper()
    scale = ru.cal_norm_scale(w.rotate_meshes(meshes), 1.8)
    assert abs(scale - float(g["norm_scale"])) <= 4 * np.finfo(np.float64).eps * float(g["norm_scale"])
    faces, texts, verts = w.prepare_side_rend(meshes, maxd=1.8)
    assert np.array_equal(faces.numpy(), g["comb_faces"]) and np.array_equal(texts.numpy(), g["comb_textures"])
    assert np.abs(verts.numpy() - g["side_verts"]).max() <= 4 * float(g["bound_side_verts"])
    assert np.array_equal(meshes[0].v, g["mesh0_v"])                # the caller's meshes are untouched
    cam = r.transform(torch.from_numpy(g["side_verts"]))
    assert np.abs(cam.numpy() - g["side_proj"]).max() <= 4 * float(g["bound_side_proj"])
    cam2 = nr.perspective(nr.look_at(torch.from_numpy(g["side_verts"]), eye), angle=30.)
    assert torch.equal(cam, cam2)


def test_projection_kinect(g):
    from chore_amd.utils import render_utils as ru
    K, ratio = ru.get_kinect_K(2048)
    assert ratio == 1.0 and np.array_equal(K.numpy(), g["kinect_K"])
    K2, ratio2 = ru.get_kinect_K(512)
    assert ratio2 == 0.25 and np.allclose(K2.numpy()[0, :2], g["kinect_K"][0, :2] * 0.25, rtol=1e-7)
    r = ru.setup_renderer(image_size=2048)
    assert r.orig_size == 2048 and r.image_size == 2048 and r.background_color == [1, 1, 1]
    proj = r.transform(torch.from_numpy(g["comb_verts"]))
    assert np.abs(proj.numpy() - g["proj"]).max() <= 4 * float(g["bound_proj"])
    with pytest.raises(NotImplementedError):
        from chore_amd.render import Renderer
        Renderer(camera_mode="look").transform(torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError):                               # no CPU rasteriser
        r.render(torch.from_numpy(g["comb_verts"]), torch.from_numpy(g["comb_faces"]), torch.from_numpy(g["comb_textures"]))


def test_align_to_input(g):
    from chore_amd.utils.render_utils import align_to_input
    info = {"rgb_newsize": (256, 192), "crop_center": np.array([40.0, 170.0]), "crop_size": np.array([150, 150])}
    assert np.array_equal(align_to_input(info, 192, _pattern(256, 256), 150, 256, False), g["align_small_rgb"])
    assert np.array_equal(align_to_input(info, 192, _pattern(256, 256)[:, :, 0], 150, 256, False, 0), g["align_small_mask"])
    info = {"rgb_newsize": (2048, 1536), "crop_center": np.array([700.0, 640.0]), "crop_size": np.array([1200, 1200])}
    big = align_to_input(info, 1536, _pattern(2048, 2048), 1200, 2048, True)
    assert big.shape == (1536, 2048, 3) and big.dtype == np.uint8
    assert np.array_equal(big[::16, ::16], g["align_mean_sample"])
    assert zlib.crc32(np.ascontiguousarray(big).tobytes()) == int(g["align_mean_crc"])


def test_load_mesh(tmp_path):
    from chore_amd.recon.recon_fit_base import write_ply
    from chore_amd.utils.render_utils import load_mesh
    rs = np.random.RandomState(0)
    v = rs.standard_normal((20, 3)).astype(np.float32)
    f = np.stack([rs.choice(20, 3, replace=False) for _ in range(30)]).astype(np.int32)
    path = str(tmp_path / "k1.smpl.ply")
    write_ply(path, v, f)
    m = load_mesh(path)
    assert np.array_equal(np.asarray(m.v, np.float32), v) and np.array_equal(np.asarray(m.f), f)
    assert load_mesh(str(tmp_path / "missing.ply")) is None


def _standin_checkout(root):
    """the files of a CHORE checkout that the drop-in import chain reads (the pattern of tests/test_assets_dropin.py), plus a
    utils/ directory with a module this package does not replace"""
    root.mkdir()
    (root / "PATHS.yml").write_text('RECON_PATH: "recon_out"\nSMPL_ASSETS_ROOT: "assets"\n')
    for pkg in ("config", "recon", "utils"):
        (root / pkg).mkdir()
    (root / "config" / "__init__.py").write_text("")
    (root / "config" / "config_loader.py").write_text('"""stand-in for the checkout\'s config loader"""\n')
    (root / "recon" / "opt_utils.py").write_text('"""stand-in for a checkout-only recon submodule"""\n')
    (root / "utils" / "__init__.py").write_text("")
    (root / "utils" / "dist_utils.py").write_text('"""stand-in for a checkout-only utils submodule"""\n')
    (root / "utils" / "render_utils.py").write_text('raise ImportError("the checkout\'s render_utils needs CUDA")\n')
    return str(root)


def test_dropin_render_aliases(tmp_path):
    """demo.py's rendering imports resolve to this package inside a CHORE checkout; utils.dist_utils stays the checkout's;
    neither cv2 nor psbody is imported"""
    ref = _standin_checkout(tmp_path / "chore")
    code = ("import sys; import chore_amd.dropin as d; d.install(); "
            "from utils.render_utils import NrWrapper; import utils.render_utils as rutils; "
            "import neural_renderer as nr; nr.Renderer; from neural_renderer.renderer import Renderer; "
            "import utils.dist_utils as du; "
            "assert Renderer is nr.Renderer and rutils.NrWrapper is NrWrapper; "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('cv2', 'psbody')]; "
            "print(NrWrapper.__module__, rutils.__file__, nr.__file__, du.__file__)")
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run([sys.executable, "-c", code], cwd=ref, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    mods = out.stdout.split()
    assert mods[0] == "chore_amd.utils.render_utils"
    assert mods[1].startswith(os.path.join(REPO, "chore_amd", "utils")) and mods[2].startswith(os.path.join(REPO, "chore_amd", "render"))
    assert mods[3].startswith(ref)


def test_render_workspace_bytes():
    from chore_amd import _lib
    ws = _lib.lib.chore_render_workspace_bytes
    base = ws(1, 1000, 256, 2)
    assert base > 0
    assert ws(1, 2000, 256, 2) > base and ws(1, 1000, 512, 2) > base and ws(2, 1000, 256, 2) > base
    sizes = [ws(1, 1000, s, 2) for s in (64, 128, 256, 512, 1024, 2048)]
    assert sizes == sorted(sizes) and all(s > 0 for s in sizes)
    faces = [ws(1, f, 2048, 2) for f in (1, 100, 30112, 60000)]
    assert faces == sorted(faces) and len(set(faces)) == 4
    # the demo view: 30 112 triangles, 2048 px at 2x: setup records + 256 bin lists of F ids
    assert 30112 * 88 + 256 * 30112 * 4 <= ws(1, 30112, 2048, 2) < 40 * 2 ** 20
    for bad in (0, 3, 4, -1):
        assert ws(1, 1000, 256, bad) == 0
    assert ws(1, 1000, 4096, 2) == 0 and ws(1, 1000, 4096, 1) > 0
