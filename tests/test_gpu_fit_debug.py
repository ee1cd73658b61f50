"""GPU: the fitter's headless debug views.  The two-frame synthetic fit of tests/test_gpu_fit_chain.py (two batches of one
frame, the shortest schedule, in the configuration that file's bit-equality test uses) with debug off and on: the fitted parameters are bit-equal, and with debug on the two PNGs
and the dense-cloud npz of every frame exist and show what they should."""
import argparse
import copy
import os

import numpy as np
import pytest
import torch

import png_ref

pytestmark = pytest.mark.gpu

FITTED = ("pose", "betas", "trans", "obj_R", "obj_t", "obj_s")


def _run(opt, out_dir, debug, use_graphs):
    """fit_recon over two batches of one frame in the configuration whose results tests/test_gpu_fit_chain.py already holds
    to bit-equality between runs (its pipelined test: fp16x3 fields, per-batch generators, the stop rule off, Adam's scalars
    on the device), with the shortest schedule: one outer iteration per phase"""
    import bench
    from chore_amd.model import CHORE
    from chore_amd.recon.assets import SyntheticAssets
    from chore_amd.recon.generator import Generator
    from chore_amd.recon.recon_fit_behave import ReconFitterBehave
    from chore_amd.utils import synth
    dev = torch.device("cuda", 0)
    o = copy.copy(opt)
    o.compute_dtype = "fp16x3"
    args = argparse.Namespace(**vars(o), save_name="test", test_kid=1, redo=True)
    net = CHORE(o).to(dev).eval()
    synth.load_synth_weights(net, seed=0)
    gen = Generator(net, None, threshold=2.0, sparse_thres=0.03, filter_val=1.0, device=dev)
    fitter = ReconFitterBehave(None, device=dev, debug=debug, obj_name="synthetic", outpath=out_dir, args=args,
                               assets=SyntheticAssets(0))
    fitter.use_graphs = fitter.reuse_graphs = use_graphs
    fitter.early_stop, fitter.adam_capturable = False, True
    fitter.batch_seed = 7                        # every batch draws from generators of its own: the two runs draw alike
    fitter.pipeline = bool(debug)                # asked to pipeline, a debug fit still runs the serial loop (the plain run's)
    fitter.smpl_iters = dict(iter_for_betas=1, iter_for_pose=1, iter_for_kpts=1, steps_per_iter=2, max_iter=1)
    fitter.object_iters = dict(obj_iter=1, joint_iter=1, steps_per_iter=2, sil_iter=1, max_iter=1)
    clouds = []
    orig_gen = gen.generate_pclouds_batch

    def recorded(*a, **kw):
        pc = orig_gen(*a, **kw)
        clouds.append({t: {k: v.detach().cpu().clone() for k, v in pc[t].items() if torch.is_tensor(v)} for t in pc})
        return pc
    gen.generate_pclouds_batch = recorded
    loader = [bench.fit_batch_inputs(1, 10 + k, dev) for k in range(2)]
    torch.manual_seed(3)
    res = fitter.fit_recon(args, loader=loader, generator=gen)
    torch.cuda.synchronize()
    assert len(res) == 2
    return [{k: r[k].detach().cpu().clone() for k in FITTED} for r in res], clouds


def _has_colour(img, colour, tol=0.035):
    """some pixel of the uint8 image is `colour` (0..1) times a shade in [0.55, 1] (ambient 0.6 .. full light)"""
    p = img.reshape(-1, 3).astype(np.float64) / 255
    c = np.asarray(colour, np.float64)
    s = (p @ c) / (c @ c)
    return bool((((s > 0.55) & (s < 1.02)) & (np.abs(p - s[:, None] * c).max(axis=1) < tol)).any())


@pytest.mark.parametrize("use_graphs", [False, True])
def test_debug_views_leave_the_fit_unchanged(opt, tmp_path, use_graphs):
    from chore_amd.utils.render_utils import PART_COLORS
    plain_dir, debug_dir = str(tmp_path / "plain"), str(tmp_path / "debug")
    plain, _ = _run(opt, plain_dir, False, use_graphs)
    debug, clouds = _run(opt, debug_dir, True, use_graphs)
    for i, (a, b) in enumerate(zip(plain, debug)):
        for k in FITTED:
            assert torch.isfinite(a[k]).all(), (i, k)
            assert torch.equal(a[k], b[k]), (i, k, float((a[k] - b[k]).abs().max()))
    assert not torch.equal(debug[0]["obj_t"], debug[1]["obj_t"])
    for i in range(2):
        folder = os.path.join(debug_dir, f"seq{10 + i}", "t0000.000", "test")
        views = {}
        for what in ("smpl", "object"):
            views[what] = png_ref.read_png(os.path.join(folder, f"k1.debug_{what}.png"))
            assert views[what].shape == (512, 512 + 640, 3) and views[what].dtype == np.uint8
            views[what] = views[what][:, 512:]          # the side view: white behind the clouds, no photo to mistake for them
        z = np.load(os.path.join(folder, "k1_densepc.npz"), allow_pickle=True)
        labels = np.unique(z["human"].item()["parts"]).astype(int)           # the parts the generator predicted for this frame
        parts = [int(k) for k in labels if _has_colour(views["smpl"], PART_COLORS[k])]
        print("frame", i, "parts predicted:", labels.tolist(), "part colours seen:", parts)
        assert len(parts) >= 3, parts
        for what in views:
            assert _has_colour(views[what], (0.0, 1.0, 0.0)), what              # the SMPL vertices
        assert _has_colour(views["object"], (1.0, 0.0, 0.0))                    # the object points
        assert sorted(z.files) == sorted(clouds[i])
        for t in clouds[i]:
            saved = z[t].item()
            assert sorted(saved) == sorted(clouds[i][t]), t
            for k in ("points", "parts"):
                if k in clouds[i][t]:
                    assert np.array_equal(saved[k], clouds[i][t][k][0].numpy()), (t, k)
        assert z["human"].item()["points"].ndim == 2 and z["human"].item()["points"].shape[1] == 3
        plain_folder = os.path.join(plain_dir, f"seq{10 + i}", "t0000.000", "test")
        assert os.path.exists(os.path.join(plain_folder, "k1.smpl.ply"))
        assert not os.path.exists(os.path.join(plain_folder, "k1.debug_smpl.png"))
        assert not os.path.exists(os.path.join(plain_folder, "k1_densepc.npz"))
