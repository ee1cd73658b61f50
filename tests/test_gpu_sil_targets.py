"""GPU: the silhouette term's targets built on the device (csrc/sil_targets.hip; SilLossROI.from_masks / set_masks / edge_loss,
chore_amd.preprocess.distance_transform_edt, ReconFitterBase.SIL_DEVICE_SETUP / SIL_EDGE_TERM) against the brute-force
restatements of tests/test_sil_targets_host.py, which that module pins to the reference's own arrays first."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from test_sil_targets_host import (crop_values, edge_edt_brute, edges_brute, edt_sq_brute, roi_intrinsics,  # noqa: F401
                                   square_boxes, targets_brute)

pytestmark = pytest.mark.gpu

# tile sizes of chore_edt_sq (csrc/sil_targets.hip; tests/test_sil_targets_host.py asserts chore_edt_tiles() returns them)
EDT_COL_TILE = 64        # columns per block of the column pass
EDT_ROW_TILE = 256       # threads per block of the row pass: a row wider than this is walked in strides
EDT_CASES = [(1, 1, 1), (1, 5, 7), (1, 7, 5), (2, 63, 65), (3, 64, 64), (1, 256, 256),
             (1, 12, EDT_COL_TILE - 1), (1, 12, EDT_COL_TILE + 1), (2, 5, EDT_ROW_TILE - 1), (2, 5, EDT_ROW_TILE + 1),
             (1, 3, 2 * EDT_ROW_TILE + 1)]


def dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a) if dt is None else np.asarray(a, dt))).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. distance transform -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edt_images(H, W):
    """the contents of one shape with their expected squares: four single corners, every pixel, one-pixel stripes both ways, a
    seeded 2 % scatter, and no feature at all (the sentinel)"""
    imgs = []
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        f = np.zeros((H, W), np.uint8)
        f[y, x] = 1
        imgs.append(f)
    imgs.append(np.ones((H, W), np.uint8))
    step = 5 if H * W <= 1 << 14 else 97         # (the brute force is O(pixels x features): fewer stripes on the large image)
    for axis in (0, 1):
        f = np.zeros((H, W), np.uint8)
        if axis:
            f[:, 2 % W::step] = 3                # any non-zero byte is a feature
        else:
            f[1 % H::step, :] = 255
        imgs.append(f)
    rs = np.random.RandomState(1000 * H + W)
    imgs.append((rs.uniform(size=(H, W)) < 0.02).astype(np.uint8))
    imgs.append(np.zeros((H, W), np.uint8))
    # (every pixel a feature: all zeros by definition -- the brute force would take pixels^2 comparisons at 256^2)
    want = [np.zeros((H, W), np.int64) if f.all() else edt_sq_brute(f) for f in imgs]
    assert np.array_equal(want[-1], np.full((H, W), 2 * max(H, W) ** 2))
    return imgs, want


@pytest.mark.parametrize("B,H,W", EDT_CASES)
def test_edt_equals_the_brute_force(B, H, W):
    """1: chore_edt_sq equal to the integer brute force at every pixel; batches mix the contents; distance_transform_edt (scipy's
    convention: distance to the nearest ZERO pixel) gives the same squares and float64 roots equal to np.sqrt bit for bit"""
    from chore_amd import _lib
    from chore_amd.preprocess import distance_transform_edt
    imgs, want = _edt_images(H, W)
    h = _lib.handle(0)
    ws = torch.empty(_lib.lib.chore_edt_workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
    n = len(imgs)
    for start in range(0, n, B):
        idx = [(start + i) % n for i in range(B)]
        feat = dev(np.stack([imgs[i] for i in idx]))
        ref = np.stack([want[i] for i in idx])
        d2 = torch.full((B, H, W), -7, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib.chore_edt_sq(h, feat.data_ptr(), B, H, W, d2.data_ptr(), ws.data_ptr(), _stream()), h, "chore_edt_sq")
        got = d2.cpu().numpy()
        assert np.array_equal(got, ref), (idx, int(np.abs(got - ref).max()), np.argwhere(got != ref)[:4])
        mask = (feat == 0).float()              # its zeros are the features
        sq = distance_transform_edt(mask, return_squared=True)
        assert sq.dtype == torch.int32 and torch.equal(sq, d2)
        root = distance_transform_edt(mask)
        assert root.dtype == torch.float64 and tuple(root.shape) == (B, H, W)
        assert np.array_equal(root.cpu().numpy().view(np.uint64), np.sqrt(ref.astype(np.float64)).view(np.uint64))
    one = distance_transform_edt((dev(imgs[0]) == 0))         # (H,W) in, (H,W) out
    assert tuple(one.shape) == (H, W) and np.array_equal(one.cpu().numpy(), np.sqrt(want[0].astype(np.float64)))


def test_edt_refuses_what_it_cannot_do():
    """H = 4097 is CHORE_EINVAL before anything is launched; CPU tensors raise"""
    from chore_amd import _lib
    from chore_amd.preprocess import distance_transform_edt
    h = _lib.handle(0)
    small = torch.zeros(64, dtype=torch.int32, device="cuda")
    for H, W in ((4097, 8), (8, 4097)):
        assert _lib.lib.chore_edt_sq(h, small.data_ptr(), 1, H, W, small.data_ptr(), small.data_ptr(), _stream()) == -1
        with pytest.raises(_lib.ChoreError):
            distance_transform_edt(torch.ones(H, W, device="cuda"))
    torch.cuda.synchronize()
    assert int(small.abs().sum()) == 0
    with pytest.raises(RuntimeError):
        distance_transform_edt(torch.ones(4, 4))


# ---- 2. reference edges and their transform ------------------------------------------------------------------------------
def test_edge_edt_reproduces_the_fixture():
    """2: chore_sil_edge_edt on the fixture's image_ref (B = 3, S = 64, kernel 7): the reference's own compute_edges and
    prepare_dist_trans (scipy) results, bit for bit -- and the brute force at kernel 3 and a power other than 1/4"""
    from chore_amd import _lib
    g = golden("sil_project.npz")
    image_ref = dev(g["image_ref"])
    B, S = image_ref.shape[:2]
    h = _lib.handle(0)
    ws = torch.empty(_lib.lib.chore_sil_edge_edt_workspace_bytes(B, S), dtype=torch.uint8, device="cuda")

    def run(k, power):
        edges, edt = torch.empty_like(image_ref), torch.empty_like(image_ref)
        _lib.check(_lib.lib.chore_sil_edge_edt(h, image_ref.data_ptr(), B, S, k, power, edges.data_ptr(), edt.data_ptr(),
                                               ws.data_ptr(), _stream()), h, "chore_sil_edge_edt")
        return edges.cpu().numpy(), edt.cpu().numpy()
    edges, edt = run(7, 0.25)
    assert np.array_equal(edges, g["ref_edges"])
    assert np.array_equal(edt.view(np.uint32), g["edt_ref_edge"].view(np.uint32))
    edges3, edt3 = run(3, 0.25)
    assert np.array_equal(edges3, edges_brute(g["image_ref"], 3))
    assert np.array_equal(edt3.view(np.uint32), edge_edt_brute(g["image_ref"], 3).view(np.uint32))
    _, edt_half = run(7, 0.5)                   # pow(d, 1): the distance itself
    d = np.stack([np.sqrt(edt_sq_brute(e > 0).astype(np.float64)) for e in g["ref_edges"]])
    np.testing.assert_allclose(edt_half, d.astype(np.float32), rtol=2.0 ** -22, atol=0)


# ---- 3. from_masks -------------------------------------------------------------------------------------------------------
CROP_CENTERS = np.array([[1000.0, 700.0], [850.5, 640.25], [1200.0, 900.0], [1017.25, 779.5]], np.float32)


@functools.lru_cache(maxsize=None)
def _masks():
    """four 512^2 object masks and a person mask that overlaps each"""
    yy, xx = np.mgrid[0:512, 0:512]
    obj = np.stack([(xx - 300) ** 2 + (yy - 210) ** 2 <= 57 ** 2,
                    (xx >= 101) & (xx <= 237) & (yy >= 77) & (yy <= 159),
                    (xx >= 470) & (yy >= 3) & (yy <= 89),
                    ((xx - 120) / 91.0) ** 2 + ((yy - 400) / 33.0) ** 2 <= 1.0]).astype(np.float32)
    person = np.stack([(xx >= 310) & (xx <= 420) & (yy >= 120) & (yy <= 330),
                       (xx - 230) ** 2 + (yy - 150) ** 2 <= 40 ** 2,
                       (xx >= 438) & (xx <= 487) & (yy >= 63) & (yy <= 197),
                       (xx >= 20) & (xx <= 110) & (yy >= 380) & (yy <= 470)]).astype(np.float32)
    return person, obj


def _template():
    g = golden("sil_project.npz")
    return g["verts"], g["faces"]


@pytest.mark.parametrize("S", [256, 64, 37])
def test_from_masks_equals_the_float64_restatement(S):
    """3: image_ref and keep_mask equal the float64 numpy crop at every pixel (no exclusion: the restatement's values keep
    more than 1e-6 from the threshold, asserted); K, the square boxes equal the host constructor's bit for bit; valid = 1; the
    distance transform is that of the brute force.  The number of crop pixels that differ from the host constructor (whose
    grid_sample runs in float32) is printed, not asserted."""
    from chore_amd.recon.obj_pose_roi import SilLossROI, make_bbox_square, mask2bbox
    person, obj = _masks()
    want_ref, want_keep, want_sq, want_valid, margin = targets_brute(person, obj, S)
    share = want_ref.mean(axis=(1, 2))
    print("S %d: min |value - 0.5| of the float64 crops %.3e, foreground share %s" % (S, margin, np.round(share, 3)))
    assert margin > 1e-6
    assert share.min() > 0.1 and share.max() < 0.6
    sil = SilLossROI.from_masks(dev(person), dev(obj), _template(), dev(CROP_CENTERS), rend_size=S)
    assert sil.valid.dtype == torch.int32 and sil.valid.tolist() == [1, 1, 1, 1] == want_valid.tolist()
    got_ref, got_keep = sil.image_ref.cpu().numpy(), sil.keep_mask.cpu().numpy()
    assert np.array_equal(got_ref, want_ref), int((got_ref != want_ref).sum())
    assert np.array_equal(got_keep, want_keep), int((got_keep != want_keep).sum())
    assert (want_keep != 1).any() and (want_keep != want_ref).any()              # the person masks do occlude
    # boxes and intrinsics: the package's own host functions, the restatement, and the host constructor
    boxes = np.stack([mask2bbox(m) for m in obj])
    sq_host = make_bbox_square(np.concatenate([boxes[:, :2], boxes[:, 2:] - boxes[:, :2]], 1), 0.3)
    assert np.array_equal(sil.box_sq.cpu().numpy().view(np.uint64), sq_host.view(np.uint64))
    assert np.array_equal(want_sq.view(np.uint64), sq_host.view(np.uint64))
    host = SilLossROI(dev(person), dev(obj), _template(), dev(CROP_CENTERS), rend_size=S)
    assert np.array_equal(sil.K.cpu().numpy().view(np.uint32), host.K.cpu().numpy().view(np.uint32))
    assert np.array_equal(roi_intrinsics(sq_host, CROP_CENTERS)[1].view(np.uint32), host.K.cpu().numpy().view(np.uint32))
    differ = int((host.image_ref != sil.image_ref).sum()) + int((host.keep_mask != sil.keep_mask).sum())
    print("S %d: %d of %d crop pixels differ between the host constructor (float32 grid_sample) and from_masks"
          % (S, differ, 2 * 4 * S * S))
    if S != 256:             # (brute force over 256^2 pixels x an outline's pixels x 4 frames: left to the two smaller sizes)
        assert np.array_equal(sil.edt_ref_edge.cpu().numpy().view(np.uint32), edge_edt_brute(want_ref, 7).view(np.uint32))
        assert np.array_equal(sil.ref_edges.cpu().numpy(), edges_brute(want_ref, 7))
    if differ == 0:          # the same crops: then the same distance transform as scipy's, bit for bit
        assert torch.equal(host.edt_ref_edge, sil.edt_ref_edge)
    for name in ("vertices", "faces", "faces32", "adj_off", "adj", "R", "t"):
        assert torch.equal(getattr(host, name), getattr(sil, name)), name


def _pose_for(centers_px, crop_centers, z=2.2):
    """identity rotation, unit scale and the translation that puts the template on the given network-input pixel"""
    u = np.asarray(centers_px, np.float64) * (1200 / 512.0) + np.asarray(crop_centers, np.float64) - 600.0
    t = np.stack([(u[:, 0] - 1018.952) / 979.7844 * z, (u[:, 1] - 779.486) / 979.840 * z, np.full(len(u), z)], 1)
    B = len(u)
    return (torch.eye(3).repeat(B, 1, 1).cuda(), dev(t, np.float32), torch.ones(B).cuda())


MASK_CENTRES = np.array([[300.0, 210.0], [169.0, 118.0], [491.0, 46.0], [120.0, 400.0]])


def test_an_empty_object_mask():
    """3 (empty frames): valid = [1, 0, 1], zero targets and a finite K for the empty frame, and a mask term equal to that of
    the two valid frames times 2/3 (the sums are pixel counts, exact in float32: one rounding each in the two means)"""
    from chore_amd.recon.obj_pose_roi import SilLossROI
    person, obj = _masks()
    S = 64
    p3, o3 = person[[0, 1, 2]].copy(), obj[[0, 1, 2]].copy()
    o3[1] = 0
    sil3 = SilLossROI.from_masks(dev(p3), dev(o3), _template(), dev(CROP_CENTERS[:3]), rend_size=S)
    sil2 = SilLossROI.from_masks(dev(p3[[0, 2]]), dev(o3[[0, 2]]), _template(), dev(CROP_CENTERS[[0, 2]]), rend_size=S)
    assert sil3.valid.tolist() == [1, 0, 1] and sil2.valid.tolist() == [1, 1]
    assert not sil3.image_ref[1].any() and not sil3.keep_mask[1].any()
    assert torch.isfinite(sil3.K).all() and torch.isfinite(sil3.edt_ref_edge).all()
    assert sil3.box_sq[1].tolist() == [0.0, 0.0, 512.0, 512.0]
    for a, b in ((0, 0), (2, 1)):
        for name in ("image_ref", "keep_mask", "K", "edt_ref_edge"):
            assert torch.equal(getattr(sil3, name)[a], getattr(sil2, name)[b]), (name, a)
    R, t, s = _pose_for(MASK_CENTRES[:3], CROP_CENTERS[:3])
    with torch.no_grad():
        l3, im3 = sil3.mask_loss(R, t, s)
        l2, im2 = sil2.mask_loss(R[[0, 2]], t[[0, 2]], s[[0, 2]])
    assert float(im2.sum()) > 50 and torch.equal(im3[[0, 2]], im2) and not im3[1].any()      # the template is in view
    l3, l2 = float(l3["mask"]), float(l2["mask"])
    print("mask term: three frames %.6f, the two valid ones %.6f" % (l3, l2))
    assert l2 > 0 and abs(l3 - l2 * 2 / 3) <= 2.0 ** -23 * l3


# ---- 4. no host round trip -----------------------------------------------------------------------------------------------
def test_set_masks_inside_a_recorded_graph():
    """4: set_masks then mask_loss captured with torch.cuda.graph (one stream: a single chain; a synchronisation or a host read
    of a device value inside would fail the capture) and replayed after other masks were written into the captured inputs:
    the buffers and the loss are those of a fresh from_masks of the new masks"""
    from chore_amd.recon.obj_pose_roi import SilLossROI
    person, obj = _masks()
    S = 64
    p_in, o_in, c_in = dev(person[:2]), dev(obj[:2]), dev(CROP_CENTERS[:2])
    sil = SilLossROI.from_masks(p_in, o_in, _template(), c_in, rend_size=S)
    R, t, s = _pose_for(MASK_CENTRES[2:], CROP_CENTERS[2:])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():               # warm-up: first launches may set kernel attributes
        sil.set_masks(p_in, o_in, c_in)
        sil.mask_loss(R, t, s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        sil.set_masks(p_in, o_in, c_in)
        loss = sil.mask_loss(R, t, s)[0]["mask"]
    before = {n: getattr(sil, n).clone() for n in ("image_ref", "keep_mask", "K", "edt_ref_edge", "valid", "box_sq")}
    p_in.copy_(dev(person[2:]))
    o_in.copy_(dev(obj[2:]))
    c_in.copy_(dev(CROP_CENTERS[2:]))
    graph.replay()
    fresh = SilLossROI.from_masks(dev(person[2:]), dev(obj[2:]), _template(), dev(CROP_CENTERS[2:]), rend_size=S)
    for n, old in before.items():
        assert torch.equal(getattr(sil, n), getattr(fresh, n)), n
        assert n == "valid" or not torch.equal(getattr(sil, n), old), n
    with torch.no_grad():
        want = fresh.mask_loss(R, t, s)[0]["mask"]
    assert float(want) > 0 and torch.equal(loss, want)


# ---- 5. edge term --------------------------------------------------------------------------------------------------------
EDGE_L = 17          # longest addition chain of chore_sil_edge_fwd for S <= 256: 8 tree levels in a block of 256 pixels, at most
#                      ceil(S^2 / 256) / 256 <= 1 partial per thread, 8 tree levels over the threads (include/chore_hip.h)
EDGE_CASES = [(1, 5), (1, 7), (3, 17), (2, 64), (1, 65)]


def _edge_case(B, S, k, binary):
    rs = np.random.RandomState(100 * S + 10 * k + binary)
    img = (rs.uniform(size=(B, S, S)) < 0.4).astype(np.float32) if binary else rs.uniform(-1, 1, (B, S, S)).astype(np.float32)
    w = rs.uniform(0, 4, (B, S, S)).astype(np.float32)
    g = rs.uniform(0.5, 2, B).astype(np.float32) * rs.choice([-1, 1], B).astype(np.float32)
    return img, w, g


@pytest.mark.parametrize("k", [7, 3])
@pytest.mark.parametrize("B,S", EDGE_CASES)
def test_edge_term_against_float64(B, S, k):
    """5: chore_sil_edge_fwd / _bwd against torch.nn.functional.max_pool2d(return_indices=True) and autograd on the CPU in
    float64: the argmax map as integers (binary images tie in every window), the sums within 2^-23 (L + 1) sum|terms| with
    L = EDGE_L, the backward within 50 x 2^-23 |g| sum_window |weight| per pixel (at most 49 additions and the product), two
    calls bit-equal, and the autograd function the same bits as the direct calls"""
    import torch.nn.functional as F
    from chore_amd import _lib
    from chore_amd.recon.obj_pose_roi import _EdgeTermFn
    assert 2.0 ** -23 * (EDGE_L + 1) <= 1e-5 and (S * S + 255) // 256 <= 256
    h = _lib.handle(0)
    for binary in (0, 1):
        img, w, g = _edge_case(B, S, k, binary)
        i64 = torch.tensor(img, dtype=torch.float64, requires_grad=True)
        w64, g64 = torch.tensor(w, dtype=torch.float64), torch.tensor(g, dtype=torch.float64)
        mp, idx = F.max_pool2d(i64[:, None], k, 1, k // 2, return_indices=True)
        terms = (mp[:, 0] - i64) * w64
        sums64 = terms.sum((1, 2))
        (sums64 * g64).sum().backward()
        abs_terms = terms.detach().abs().sum((1, 2)).numpy()
        win = F.avg_pool2d(w64[:, None].abs(), k, 1, k // 2, count_include_pad=True, divisor_override=1)[:, 0].numpy()
        d_img, d_w, d_g = dev(img), dev(w), dev(g)
        ws = torch.empty(_lib.lib.chore_sil_edge_workspace_bytes(B, S), dtype=torch.uint8, device="cuda")
        runs = []
        for _ in range(2):
            sums = torch.full((B,), float("nan"), device="cuda")
            arg = torch.full((B, S, S), -1, dtype=torch.int32, device="cuda")
            gi = torch.full((B, S, S), float("nan"), device="cuda")
            _lib.check(_lib.lib.chore_sil_edge_fwd(h, d_img.data_ptr(), d_w.data_ptr(), B, S, k, sums.data_ptr(), arg.data_ptr(),
                                                   ws.data_ptr(), _stream()), h, "chore_sil_edge_fwd")
            _lib.check(_lib.lib.chore_sil_edge_bwd(h, d_w.data_ptr(), arg.data_ptr(), d_g.data_ptr(), B, S, k, gi.data_ptr(),
                                                   _stream()), h, "chore_sil_edge_bwd")
            runs.append((sums.cpu().numpy(), arg.cpu().numpy(), gi.cpu().numpy()))
        (sums, arg, gi), again = runs
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], again)), "two calls differ"
        assert np.array_equal(arg.astype(np.int64), idx[:, 0].numpy()), (binary, int((arg != idx[:, 0].numpy()).sum()))
        err = np.abs(sums.astype(np.float64) - sums64.detach().numpy())
        bound = 2.0 ** -23 * (EDGE_L + 1) * abs_terms
        print("B %d S %d k %d binary %d: sums %s, |error| %s, bound %s" % (B, S, k, binary, sums, err, bound))
        assert (err <= bound).all()
        gerr = np.abs(gi.astype(np.float64) - i64.grad.numpy())
        gbound = 50 * 2.0 ** -23 * np.abs(g.astype(np.float64))[:, None, None] * win
        print("  backward: largest |error| / bound %.3e" % float((gerr / np.maximum(gbound, 1e-300)).max()))
        assert (gerr <= gbound).all()
        leaf = d_img.clone().requires_grad_(True)
        out = _EdgeTermFn.apply(leaf, d_w, k)
        out.backward(d_g)
        assert np.array_equal(out.detach().cpu().numpy(), sums) and np.array_equal(leaf.grad.cpu().numpy(), gi)


def test_edge_loss_of_the_term():
    """5 (the module): edge_loss(image) = mean_b sum (compute_edges(image) * edt_ref_edge), forward() keeps its five values"""
    from chore_amd.recon.obj_pose_roi import SilLossROI
    person, obj = _masks()
    sil = SilLossROI.from_masks(dev(person[:2]), dev(obj[:2]), _template(), dev(CROP_CENTERS[:2]), rend_size=64)
    R, t, s = _pose_for(MASK_CENTRES[:2], CROP_CENTERS[:2])
    t = t.requires_grad_(True)
    out = sil(R, t, s)
    assert len(out) == 5 and list(out[0]) == ["mask"]
    image = out[1]
    edge = sil.edge_loss(image)
    assert list(edge) == ["edge"] and edge["edge"].dim() == 0 and edge["edge"].dtype == torch.float32
    want = float((out[2].detach().double() * out[4].double()).sum((1, 2)).mean())
    assert want > 0 and abs(float(edge["edge"].detach()) - want) <= 1e-5 * want
    edge["edge"].backward()
    assert torch.isfinite(t.grad).all()


# ---- 6. fitter -----------------------------------------------------------------------------------------------------------
def _fit_objects(opt, net=None, flip=False):
    """B = 2 frames of the fixture's 40-vertex template in front of a rigid body (the pieces of tests/fit_harness.py), with the
    512^2 masks of _masks() in the images' channels 3 and 4; flip: another batch (the other two masks)"""
    import copy
    from chore_amd.lib_smpl.priors import synthetic_priors
    from chore_amd.lib_smpl.wrapper_pytorch import SMPLPyTorchWrapperBatch
    from chore_amd.model import CHORE
    from chore_amd.recon.recon_fit_behave import ReconFitterBehave
    from chore_amd.utils import synth
    from fit_harness import fit_case, smplh_faces
    from test_gpu_query import nhwc
    B = 2
    c = fit_case(B)
    if net is None:
        o = copy.copy(opt)
        o.compute_dtype = "fp32"
        net = CHORE(o).cuda().eval()
        synth.load_synth_weights(net, seed=0)
        for p in net.parameters():
            p.requires_grad_(False)
        net.im_feat_list = [nhwc(c["feat"])]
        net.tmpx = nhwc(c["tmpx"])
    model = synth.synth_smplh_model(0)
    model["f"] = smplh_faces()
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy())      # noqa: E731
    smpl = SMPLPyTorchWrapperBatch(model, B, betas=t_(c["betas"]), pose=t_(c["pose"]), trans=t_(c["trans"])).cuda()
    body_prior, hand_prior = synthetic_priors(0)
    labels = torch.from_numpy(c["labels"]).cuda()
    verts, faces = _template()
    fitter = ReconFitterBehave.from_parts(device="cuda:0", part_labels=labels, body_prior=body_prior, hand_prior=hand_prior,
                                          scan_verts=verts, scan_faces=faces)
    fitter.adam_capturable = True
    fitter.SIL_DEVICE_SETUP = fitter.SIL_EDGE_TERM = True
    fitter.SIL_REND_SIZE = 64
    person, obj = _masks()
    pick = [2, 3] if flip else [0, 1]
    images = np.zeros((B, 5, 512, 512), np.float32)
    images[:, 3], images[:, 4] = person[pick], obj[pick]
    cc = CROP_CENTERS[pick]
    _, t0, _ = _pose_for(MASK_CENTRES[pick] + np.array([9.0, -6.0]), cc)            # starts a few pixels off the mask
    rs = np.random.RandomState(3)
    pts = verts[rs.randint(0, len(verts), 3000)]
    data = dict(net=net, query_dict={"crop_center": dev(cc)}, part_labels=labels.unsqueeze(0).repeat(B, 1), smpl=smpl,
                objects=dev(np.stack([pts] * B), np.float32), images=dev(images),
                obj_R=t_(c["obj_R"]).cuda().requires_grad_(True), obj_t=t0.clone().requires_grad_(True),
                obj_s=torch.ones(B).cuda().requires_grad_(True))
    return fitter, net, data


def _run(fitter, net, data, log=None):
    if log is not None:
        orig = fitter.forward_step

        def f(*a, **k):
            ld = orig(*a, **k)
            log.append({k_: v.detach() for k_, v in ld.items()})
            return ld
        fitter.forward_step = f
    torch.manual_seed(12)
    _, R, t = fitter.optimize_smpl_object(net, data, obj_iter=1, joint_iter=0, steps_per_iter=3, sil_iter=2, max_iter=0)
    return [x.detach().clone() for x in (R, t, data["obj_s"])]


def test_fitter_with_device_setup_and_edge_term(opt):
    """6: a short 'object only' + 'sil' schedule with SIL_DEVICE_SETUP = SIL_EDGE_TERM = True: loss_dict carries a finite
    "edge"; the fitted obj_R / t / s are bit-equal between eager steps and recorded graphs; a second batch run through the
    kept slot (set_masks on the kept term) is bit-equal to a fresh fitter on that batch"""
    from chore_amd.recon.obj_pose_roi import SilLossROI
    log = []
    eager, net, data = _fit_objects(opt)
    res_eager = _run(eager, net, data, log)
    sil_steps = [ld for ld in log if "mask" in ld]
    assert len(sil_steps) >= 6 and all("edge" in ld and list(ld)[-1] == "edge" for ld in sil_steps)
    edge = torch.stack([ld["edge"] for ld in sil_steps])
    print("edge term per 'sil' step:", edge.tolist(), " mask:", [float(ld["mask"]) for ld in sil_steps])
    assert torch.isfinite(edge).all() and float(edge.max()) > 0
    assert isinstance(data["silhouette"], SilLossROI) and data["silhouette"].valid.tolist() == [1, 1]
    assert tuple(data["silhouette"].image_ref.shape) == (2, 64, 64)
    assert float(eager.get_loss_weights()["edge"](1.0, 0)) == 0.003 ** 2
    graphed, _, data = _fit_objects(opt, net=net)
    graphed.use_graphs = True
    res_graph = _run(graphed, net, data)
    for name, a, b in zip(("R", "t", "s"), res_eager, res_graph):
        print("eager vs graph %s: largest difference %.3e" % (name, float((a - b).abs().max())))
    for name, a, b in zip(("R", "t", "s"), res_eager, res_graph):
        assert torch.isfinite(b).all() and torch.equal(a, b), name
    # the kept slot: batch 1 records, batch 2 replays on the kept term refreshed by set_masks
    keeper, _, data = _fit_objects(opt, net=net)
    keeper.use_graphs = keeper.reuse_graphs = True
    first = _run(keeper, net, data)
    kept_sil = data["silhouette"]
    for a, b in zip(first, res_graph):
        assert torch.equal(a, b)
    _, _, data2 = _fit_objects(opt, net=net, flip=True)
    second = _run(keeper, net, data2)
    assert data2["silhouette"] is kept_sil and len(keeper._slots) == 1
    fresh, _, data3 = _fit_objects(opt, net=net, flip=True)
    fresh.use_graphs = True
    want = _run(fresh, net, data3)
    for name, a, b in zip(("R", "t", "s"), second, want):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert not torch.equal(second[1], first[1])
    for n in ("image_ref", "keep_mask", "K", "edt_ref_edge"):
        assert torch.equal(getattr(kept_sil, n), getattr(data3["silhouette"], n)), n


def test_switches_are_off_by_default():
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    from chore_amd.recon.recon_fit_coco import ReconFitterCoco
    assert ReconFitterBase.SIL_DEVICE_SETUP is False and ReconFitterBase.SIL_EDGE_TERM is False
    f = ReconFitterCoco.from_parts(device="cuda:0")
    assert "edge" not in f.get_loss_weights()
    f.SIL_EDGE_TERM = True
    assert float(f.get_loss_weights()["edge"](1.0, 0)) == float(f.get_loss_weights()["mask"](1.0, 0))
