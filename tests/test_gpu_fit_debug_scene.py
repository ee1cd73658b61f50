"""GPU: the fitter's scene view.  The two-frame synthetic fit of tests/test_gpu_fit_debug.py with debug off and on: the fitted
parameters are bit-equal, and with debug on every frame additionally has k1.debug_fit.png -- the fitted meshes together with
the clouds they were fitted to (ReconFitterBase.visualize_fit_scene) -- next to the two cloud views."""
import os

import numpy as np
import pytest
import torch

import png_ref
from test_gpu_fit_debug import FITTED, _has_colour, _run

pytestmark = pytest.mark.gpu


def _under_opacity(side, opacity):
    """the side view with a translucent layer over its WHITE background undone: where a face of opacity o shows the
    background the pixel is o * m + (1 - o) * 1, so (pixel - (1 - o)) / o is the lit mesh colour m again (scaled to 0..255 for
    _has_colour; the uint8 rounding grows by 1 / o, far below its tolerance)"""
    return (side.astype(np.float64) / 255 - (1 - opacity)) / opacity * 255


def test_scene_view_of_the_fit(opt, tmp_path):
    from chore_amd.recon.recon_fit_base import ReconFitterBase as Fitter
    from chore_amd.utils.render_utils import PART_COLORS, SMPL_OBJ_COLOR_LIST
    plain_dir, debug_dir = str(tmp_path / "plain"), str(tmp_path / "debug")
    plain, _ = _run(opt, plain_dir, False, False)
    debug, _ = _run(opt, debug_dir, True, False)
    for i, (a, b) in enumerate(zip(plain, debug)):
        for k in FITTED:
            assert torch.isfinite(a[k]).all(), (i, k)
            assert torch.equal(a[k], b[k]), (i, k, float((a[k] - b[k]).abs().max()))
    assert 0 < Fitter.VIEW_MESH_OPACITY < 1 and 0 < Fitter.VIEW_GT_OPACITY < 1 and Fitter.VIEW_POINT_BIAS >= 0
    for i in range(2):
        folder = os.path.join(debug_dir, f"seq{10 + i}", "t0000.000", "test")
        view = png_ref.read_png(os.path.join(folder, "k1.debug_fit.png"))
        assert view.shape == (512, 512 + 640, 3) and view.dtype == np.uint8
        side = view[:, 512:]                     # white behind the scene, no photo to mistake for it
        meshes = _under_opacity(side, Fitter.VIEW_MESH_OPACITY)
        for what, colour in zip(("SMPL mesh", "object mesh"), SMPL_OBJ_COLOR_LIST):
            assert _has_colour(meshes, colour), (i, what)
        z = np.load(os.path.join(folder, "k1_densepc.npz"), allow_pickle=True)
        labels = np.unique(z["human"].item()["parts"]).astype(int)           # the parts the generator predicted for this frame
        parts = [int(k) for k in labels if _has_colour(side, PART_COLORS[k])]
        centres = [c for c in (Fitter.VIEW_CYAN, Fitter.VIEW_YELLOW, Fitter.VIEW_MAGENTA) if _has_colour(side, c)]
        print("frame", i, "parts predicted:", labels.tolist(), "part colours seen:", parts, "centre colours seen:", centres)
        assert len(parts) >= 3, parts
        assert _has_colour(side, (1.0, 0.0, 0.0))                               # the generator's object points
        assert centres
        assert (view[:, :512] != view[:, :512][0, 0]).any()                     # the input view is not blank
        for what in ("smpl", "object"):
            assert os.path.exists(os.path.join(folder, f"k1.debug_{what}.png")), what
        plain_folder = os.path.join(plain_dir, f"seq{10 + i}", "t0000.000", "test")
        assert os.path.exists(os.path.join(plain_folder, "k1.smpl.ply"))
        assert not os.path.exists(os.path.join(plain_folder, "k1.debug_fit.png"))
