"""GPU: the training image preparation (csrc/image_prep.hip: chore_prep_blur_u8, chore_prep_train_compose;
chore_amd/data/train_image_prep.py) against tests/train_image_ref.py -- PIL's GaussianBlur restated (pinned against PIL and
against BaseDataset.blur_image's fixture by tests/test_train_image_host.py) and the crop / resize / compose of
oracle/image_prep.py.  Integer arithmetic: exact equality throughout."""
import os

import numpy as np
import pytest
import torch

from oracle import image_prep as oi
from train_image_ref import box_params_ref, pil_blur_ref, train_crop_ref

pytestmark = pytest.mark.gpu


def _prep(**kw):
    from chore_amd.data import TrainImagePrep
    return TrainImagePrep(**kw)


def _blur(prep, imgs, radii):
    """imgs (B,H,W,C) numpy through chore_prep_blur_u8 with one radius per image"""
    prm, max_r = prep._params(radii)
    out = prep.blur(torch.from_numpy(imgs).cuda(), torch.from_numpy(prm).cuda(), max_r)
    return out.cpu().numpy()


def _radius_with_box(R):
    """a PIL radius whose box radius has integer part R"""
    for r in np.arange(R - 2.0, R + 4.0, 0.05):
        if box_params_ref(r)[1] == R:
            return float(r)
    raise AssertionError(R)


@pytest.mark.parametrize("shape", [(37, 53, 3), (64, 48, 1), (5, 300, 4)])
def test_blur_three_radii_in_one_call(shape):
    """odd sizes (byte-wise staging), one and four channels, more than one strip and row block, a copy beside two blurs;
    12.75 has R = 12 > the 5-px side of the third shape"""
    rs = np.random.RandomState(shape[0])
    imgs = rs.randint(0, 256, (3,) + shape).astype(np.uint8)
    radii = [0, 0.9, 12.75]
    got = _blur(_prep(), imgs, radii)
    for b, r in enumerate(radii):
        want = pil_blur_ref(imgs[b, :, :, 0] if shape[2] == 1 else imgs[b], r).reshape(shape)
        assert np.array_equal(got[b], want), (shape, r, np.argwhere(got[b] != want)[:4])
    assert np.array_equal(got[0], imgs[0])


def test_blur_window_wider_than_the_image():
    imgs = np.random.RandomState(4).randint(0, 256, (1, 37, 53, 3)).astype(np.uint8)
    assert box_params_ref(40)[1] == 39 > 37
    assert np.array_equal(_blur(_prep(), imgs, [40])[0], pil_blur_ref(imgs[0], 40))


def test_blur_at_and_above_the_cap():
    from chore_amd import _lib
    prep = _prep()
    cap = int(_lib.lib.chore_prep_blur_max_radius())
    assert cap >= 32
    imgs = np.random.RandomState(5).randint(0, 256, (1, 24, 40, 3)).astype(np.uint8)
    r = _radius_with_box(cap)
    assert np.array_equal(_blur(prep, imgs, [r])[0], pil_blur_ref(imgs[0], r))
    above = _radius_with_box(cap + 1)
    with pytest.raises(ValueError):
        prep.blur_image(imgs[0], above)
    with pytest.raises(ValueError):
        prep.prepare(imgs, imgs[..., 0], imgs[..., 0], flip=[False], blur_radius=[above])
    # the C entry point refuses it too, with a message, and launches nothing
    x = torch.from_numpy(imgs).cuda()
    with pytest.raises(_lib.ChoreError, match="above the supported"):
        prep.blur(x, torch.zeros(1, 3, dtype=torch.int32, device="cuda"), cap + 1)
    with pytest.raises(ValueError):
        prep.blur(x.float(), torch.zeros(1, 3, dtype=torch.int32, device="cuda"), 0)


def test_blur_equals_the_reference_fixture():
    """what BaseDataset.blur_image itself made (tests/golden/make_train_image_golden.py)"""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "train_image_prep.npz"))
    n = len(g["radius"])
    got = _blur(_prep(), np.stack([g["image"]] * n), list(g["radius"]))
    assert np.array_equal(got, g["blurred"])
    prep = _prep(phase="val", aug_blur=float(g["aug_blur"][2]), seed=int(g["blur_seed"][2]))
    assert np.array_equal(prep.blur_image(g["image"]), g["blurred"][2])          # radius drawn like the reference's
    assert np.array_equal(prep.blur_image(g["image"][..., 1], float(g["radius"][1])), pil_blur_ref(g["image"][..., 1], g["radius"][1]))


def _scene(rs, B, H, W):
    rgb = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    pm = rs.randint(0, 256, (B, H, W)).astype(np.uint8)          # soft values on both sides of 127.5: the masking is exercised
    om = rs.randint(0, 256, (B, H, W)).astype(np.uint8)
    return rgb, pm, om


@pytest.mark.parametrize("S", [32, 64])
def test_compose_matches_the_reference(S):
    """(96,128) images, crop 64 -> S = 32 (the exact 2 x 2 path) and 64 (the copy path); centres interior, at the top-left
    corner, overhanging right and bottom; flips 0 1 0 1; radii 0 and not"""
    rs = np.random.RandomState(S)
    rgb, pm, om = _scene(rs, 4, 96, 128)
    centers = np.array([[60, 50], [3, 2], [120, 40], [70, 93]])
    flips, radii = [False, True, False, True], [0.0, 1.7, 0.9, 0.0]
    prep = _prep(image_size=(S, S), crop_size=64)
    prm, max_r = prep._params(radii)
    blurred = prep.blur(torch.from_numpy(rgb).cuda(), torch.from_numpy(prm).cuda(), max_r)
    got = prep.compose(blurred, torch.from_numpy(pm).cuda(), torch.from_numpy(om).cuda(), prep.crop_corners(centers), flips).cpu().numpy()
    assert got.shape == (4, 5, S, S) and got.dtype == np.float32
    for b in range(4):
        want = train_crop_ref(rgb[b], pm[b], om[b], centers[b], flips[b], radii[b], (S, S), 64)
        assert np.array_equal(got[b], want), (S, b, np.abs(got[b] - want).max())
    assert not np.array_equal(got[1], train_crop_ref(rgb[1], pm[1], om[1], centers[1], False, radii[1], (S, S), 64))


def test_compose_bilinear_path_and_single_image_entry_point():
    """crop 60 -> S = 32: the general 11-bit bilinear path; and B = 1 without a mirror is chore_prep_crop_compose bit for bit"""
    from chore_amd import _lib
    rs = np.random.RandomState(9)
    rgb, pm, om = _scene(rs, 2, 96, 128)
    centers = np.array([[100, 80], [64, 48]])
    prep = _prep(image_size=(32, 32), crop_size=60)
    d = [torch.from_numpy(a).cuda() for a in (rgb, pm, om)]
    tlbr = prep.crop_corners(centers)
    got = prep.compose(d[0], d[1], d[2], tlbr, [True, False]).cpu().numpy()
    for b, f in enumerate([True, False]):
        assert np.array_equal(got[b], train_crop_ref(rgb[b], pm[b], om[b], centers[b], f, 0.0, (32, 32), 60)), b
    one = prep.compose(d[0][1:], d[1][1:], d[2][1:], tlbr[1:], [False])
    single = torch.empty(5, 32, 32, dtype=torch.float32, device="cuda")
    h, s = prep._call()
    t = [int(v) for v in tlbr[1]]
    _lib.check(_lib.lib.chore_prep_crop_compose(h, d[0][1].data_ptr(), d[1][1].data_ptr(), d[2][1].data_ptr(), 96, 128, t[0], t[1],
                                                t[2], t[3], 32, single.data_ptr(), s), h, "chore_prep_crop_compose")
    assert torch.equal(one[0], single) and np.array_equal(got[1], single.cpu().numpy())


def _full_scene():
    rs = np.random.RandomState(21)
    B, H, W = 2, 1536, 2048
    rgb = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    pm, om = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
    pm[0, 300:1200, 800:1100], om[0, 700:1000, 1050:1400] = 255, 255
    pm[0, 300:304, 800:1100] = rs.randint(90, 200, (4, 300))
    pm[1, 900:1500, 1500:1900], om[1, 1200:1530, 1800:2040] = 255, 255        # the crop overhangs right and bottom
    return rgb, pm, om


@pytest.fixture(scope="module")
def full():
    """one full-size batch through prepare (flip + blur drawn from seed 3) and its reference, computed once"""
    rgb, pm, om = _full_scene()
    dev = [torch.from_numpy(a).cuda() for a in (rgb, pm, om)]
    kw = dict(image_size=(512, 512), crop_size=1200, random_flip=True, aug_blur=0.05, seed=3)
    out = _prep(**kw).prepare(*dev)
    centers = []
    for b in range(2):
        bmin, bmax = oi.masks2bbox([pm[b], om[b]])
        centers.append((bmin + bmax) // 2)
    ref = np.stack([train_crop_ref(rgb[b], pm[b], om[b], centers[b], out["flip"][b], out["blur_radius"][b], (512, 512), 1200)
                    for b in range(2)])
    return dict(dev=dev, kw=kw, out=out, centers=np.stack(centers), ref=ref)


def test_prepare_full_size_batch(full):
    out = full["out"]
    # seed 3 mirrors one of the two items and blurs both, one of them with R >= 4
    assert list(out["flip"]) == [True, False] or list(out["flip"]) == [False, True]
    assert (out["blur_radius"] > 0).all() and out["blur_radius"].max() > 5
    assert out["images"].shape == (2, 5, 512, 512) and out["images"].dtype == torch.float32 and out["images"].is_cuda
    assert out["crop_center"].dtype == torch.float32 and np.array_equal(out["crop_center"].cpu().numpy(), full["centers"])
    got = out["images"].cpu().numpy()
    assert np.array_equal(got, full["ref"]), np.abs(got - full["ref"]).max()
    # same seed, same bits
    again = _prep(**full["kw"]).prepare(*full["dev"])
    assert torch.equal(again["images"], out["images"]) and np.array_equal(again["blur_radius"], out["blur_radius"])
    # the reference's method on one item: its mirror given, its radius drawn
    prep = _prep(**full["kw"])
    img0, c0 = prep.prepare_image_crop(full["dev"][0][0], full["dev"][1][0], full["dev"][2][0], True)
    assert img0.shape == (5, 512, 512) and img0.dtype == np.float32 and np.array_equal(c0, full["centers"][0])


def test_graph_replay_is_bit_equal(full):
    """the two kernels of the blur and the compose launch recorded into a hipGraph: no host read, no allocation"""
    prep = _prep(**full["kw"])
    rgb, pm, om = full["dev"]
    out = full["out"]
    prm, max_r = prep._params(out["blur_radius"])
    prm = torch.from_numpy(prm).cuda()
    tlbr = prep.crop_corners(full["centers"])
    ws, blurred = prep.blur_workspace(rgb.shape), torch.empty_like(rgb)
    images = torch.empty(2, 5, 512, 512, dtype=torch.float32, device="cuda")

    def launch():
        prep.blur(rgb, prm, max_r, out=blurred, workspace=ws)
        prep.compose(blurred, pm, om, tlbr, out["flip"], out=images)
    launch()
    torch.cuda.synchronize()
    assert torch.equal(images, out["images"])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    images.zero_()
    blurred.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(images, out["images"])


def test_model_filter_runs_on_prepared_images(full, opt):
    from chore_amd.model import CHORE
    from chore_amd.utils import synth
    net = CHORE(opt).cuda().eval()
    synth.load_synth_weights(net, seed=0)
    with torch.no_grad():
        net.filter(full["out"]["images"])
    feat = net.im_feat_list[-1]
    assert feat.shape[0] == 2 and torch.isfinite(feat.float()).all()
