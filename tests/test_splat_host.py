"""CPU: what the point-cloud views need on the host -- the PNG writer, the world-radius formula, the agreement of the two
numpy restatements of the splat rule on the inputs of the GPU tests, and the fitter's visualisation surface."""
import inspect
import math

import numpy as np
import pytest
import torch

import png_ref
import splat_ref


@pytest.mark.parametrize("shape", [(5, 7, 3), (3, 9), (1, 1, 3), (11, 3, 1), (33, 17)])
def test_write_png_round_trip(shape, tmp_path):
    from chore_amd.utils.render_utils import write_png
    a = np.random.RandomState(sum(shape)).randint(0, 256, shape).astype(np.uint8)
    f = str(tmp_path / "a.png")
    write_png(f, a)
    want = a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a
    assert np.array_equal(png_ref.read_png(f), want)
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.open(f)), want)


def test_write_png_refuses_what_it_cannot_write(tmp_path):
    from chore_amd.utils.render_utils import write_png
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "b.png"), bad)


def test_world_radius_to_pixels_by_hand():
    """focal_px * world_radius / z: the Kinect K scaled to the rendering in projection mode, (size / 2) / tan(angle) in look_at"""
    from chore_amd.render import Renderer, world_radius_to_pixels
    from chore_amd.utils.render_utils import get_kinect_K, setup_side_renderer
    K, ratio = get_kinect_K(1024)
    r = Renderer(image_size=1024, K=K, R=torch.eye(3)[None], t=torch.zeros(1, 3), orig_size=2048 * ratio)
    focal = r.focal_pixels()
    assert focal.shape == (1,) and abs(float(focal) - 979.784 / 2) < 1e-3
    assert abs(float(world_radius_to_pixels(0.06, 2.2, focal)) - 979.784 / 2 * 0.06 / 2.2) < 1e-4      # 13.36 px
    half = Renderer(image_size=512, K=K, R=torch.eye(3)[None], t=torch.zeros(1, 3), orig_size=2048 * ratio)
    assert abs(float(half.focal_pixels()) - 979.784 / 4) < 1e-3               # the same K drawn at half the size
    side = setup_side_renderer(2.0, 0., 90.)
    f = side.focal_pixels()
    assert abs(f - 320 / math.tan(math.radians(30))) < 1e-9                    # 554.26 px
    assert abs(world_radius_to_pixels(0.008, 2.0, f) - 554.2562584 * 0.008 / 2.0) < 1e-6
    z = torch.tensor([[1.0, 2.0, 4.0]])
    assert torch.allclose(world_radius_to_pixels(torch.tensor(0.1), z, f), torch.tensor([[55.42562584, 27.71281292, 13.85640646]]))


@pytest.mark.parametrize("size,ssaa", splat_ref.ISSUE_GRIDS)
def test_float32_and_float64_restatements_agree(size, ssaa):
    """the winner maps of the two restatements on the clouds of tests/test_gpu_splat.py: no sample differs (the value tests
    there tolerate 0.5 % of the covered samples)"""
    pts, col, rad = splat_ref.issue_cloud(0, ssaa=ssaa)
    for radius in (rad, 1.7):
        a = splat_ref.splat(pts, col, radius, size, ssaa, dtype=np.float32)
        b = splat_ref.splat(pts, col, radius, size, ssaa, dtype=np.float64)
        assert a["rgb"].dtype == np.float32 and b["rgb"].dtype == np.float64
        assert (a["index"] >= 0).any() and (a["index"] < 0).any()
        assert (a["index"] != b["index"]).sum() == 0


def test_restatement_rule_by_hand():
    """one point at the centre of sample (5, 2) of an 8 x 8 grid, radius 1 sample: the plus-shaped five samples, the centre
    at full brightness, the arms at the ambient term; row 2 of the samples is row 5 of the flipped output"""
    S = 8
    pts = np.array([[[(2 * 5 + 1 - S) / S, (2 * 2 + 1 - S) / S, 1.0]]], np.float32)
    out = splat_ref.splat(pts, np.array([[[1.0, 0.5, 0.0]]], np.float32), 1.0, S, 1, ambient=0.25, background=(0, 0, 1))
    want = np.full((S, S), -1)
    want[2, 5] = want[1, 5] = want[3, 5] = want[2, 4] = want[2, 6] = 0
    assert np.array_equal(out["index"][0], want)
    assert np.allclose(out["rgb"][0, :, 5, 5], (1.0, 0.5, 0.0)) and np.allclose(out["rgb"][0, :, 5, 4], (0.25, 0.125, 0.0))
    assert np.array_equal(out["rgb"][0, :, 0, 0], (0, 0, 1)) and out["depth"][0, 0, 0] == 100 and out["alpha"][0, 5, 5] == 1


def test_fitter_visualisation_surface():
    """the reference's names and parameter lists (recon/recon_fit_base.py:442, 704, 749, 798)"""
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    want = {"visualize_smpl_fit": ["self", "data_dict", "smpl", "smpl_verts"],
            "visualize_fitting": ["self", "data_dict", "object", "smpl", "smpl_verts"],
            "visualize_contact_fitting": ["self", "data_dict", "edges", "image", "model", "obj_center_pred", "object", "smpl",
                                          "smpl_verts"],
            "save_neural_recon": ["self", "train_paths", "recon_batch", "save_name", "tid"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(ReconFitterBase, name)).parameters) == params, name


def test_save_neural_recon_layout(tmp_path):
    import os
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    fitter = ReconFitterBase.from_parts(device="cpu")
    fitter.outpath = str(tmp_path)
    batch = {"human": {"points": torch.arange(24.).reshape(2, 4, 3), "parts": torch.arange(8).reshape(2, 4)},
             "object": {"points": torch.ones(2, 5, 3), "pca_axis": torch.eye(3).repeat(2, 1, 1)}}
    paths = [os.path.join("in", "seq0", f"t{i}", "k1.color.jpg") for i in range(2)]
    files = fitter.save_neural_recon(paths, batch, "name", 3)
    assert files == [os.path.join(str(tmp_path), "seq0", f"t{i}", "name", "k3_densepc.npz") for i in range(2)]
    for i, f in enumerate(files):
        z = np.load(f, allow_pickle=True)
        assert sorted(z.files) == ["human", "object"]
        human, obj = z["human"].item(), z["object"].item()
        assert np.array_equal(human["points"], batch["human"]["points"][i].numpy()) and human["parts"].shape == (4,)
        assert obj["pca_axis"].shape == (3, 3) and obj["points"].shape == (5, 3)
