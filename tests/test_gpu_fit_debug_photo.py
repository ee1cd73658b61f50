"""GPU: the fitter's photo view.  The two-frame synthetic fit of tests/test_gpu_fit_debug.py with debug off, and with debug and
VIEW_PHOTO_TEXTURES on: the fitted parameters are bit-equal, and every frame of the debug run has k1.debug_photo.png."""
import os

import numpy as np
import pytest
import torch

import png_ref
from test_gpu_fit_debug import FITTED, _run

pytestmark = pytest.mark.gpu


def test_photo_view_of_the_fit(opt, tmp_path, monkeypatch):
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    plain_dir, debug_dir = str(tmp_path / "plain"), str(tmp_path / "debug")
    plain, _ = _run(opt, plain_dir, False, False)
    monkeypatch.setattr(ReconFitterBase, "VIEW_PHOTO_TEXTURES", True)
    debug, _ = _run(opt, debug_dir, True, False)
    for i, (a, b) in enumerate(zip(plain, debug)):
        for k in FITTED:
            assert torch.isfinite(a[k]).all(), (i, k)
            assert torch.equal(a[k], b[k]), (i, k, float((a[k] - b[k]).abs().max()))
    for i in range(2):
        folder = os.path.join(debug_dir, f"seq{10 + i}", "t0000.000", "test")
        view = png_ref.read_png(os.path.join(folder, "k1.debug_photo.png"))
        assert view.shape == (512, 512 + 640, 3) and view.dtype == np.uint8
        assert (view[:, :512] != view[:, :512][0, 0]).any()                     # the photo
        side = view[:, 512:]
        assert (side != 255).any(1).sum() > 50                                  # the meshes, over the white background
        for what in ("smpl", "object", "fit"):
            assert os.path.exists(os.path.join(folder, f"k1.debug_{what}.png")), what
        assert not os.path.exists(os.path.join(plain_dir, f"seq{10 + i}", "t0000.000", "test", "k1.debug_photo.png"))
