"""CPU: the yardsticks of tests/test_gpu_sil_targets.py, pinned to the reference before any kernel is compared with them.

The restatements below are brute force on purpose -- integers, O(pixels x features) -- and are what the GPU tests compare the
kernels of csrc/sil_targets.hip against.  tests/golden/sil_project.npz was written by the reference's own code (its
compute_edges, its prepare_dist_trans with scipy's distance_transform_edt, PHOSA's make_bbox_square, to_original_bbox,
compute_K_roi): the restatements must reproduce its arrays bit for bit."""
import numpy as np

from conftest import golden


# ---- restatements --------------------------------------------------------------------------------------------------------
def edt_sq_brute(feature, sentinel=None):
    """(H,W) array -> int64 (H,W): squared distance from every pixel to the nearest pixel with feature != 0, by comparing every
    pixel with every feature pixel; `sentinel` (default 2 max(H,W)^2, the kernel's documented value) where there is none"""
    feature = np.asarray(feature)
    H, W = feature.shape
    fy, fx = np.nonzero(feature)
    if fy.size == 0:
        return np.full((H, W), 2 * max(H, W) ** 2 if sentinel is None else sentinel, np.int64)
    py, px = np.divmod(np.arange(H * W, dtype=np.int64), W)
    out = np.empty(H * W, np.int64)
    step = max(1, (1 << 22) // fy.size)
    for i in range(0, H * W, step):
        dy = py[i:i + step, None] - fy[None, :].astype(np.int64)
        dx = px[i:i + step, None] - fx[None, :].astype(np.int64)
        out[i:i + step] = (dy * dy + dx * dx).min(1)
    return out.reshape(H, W)


def maxpool_brute(img, k):
    """(S,S) float array -> (max over the k x k window, index y * S + x of its first maximum in row-major order); stride 1,
    padding k // 2 that never wins (torch.max_pool2d's rule)"""
    img = np.asarray(img)
    S = img.shape[0]
    r = k // 2
    best = np.full((S, S), -np.inf, img.dtype)
    arg = np.full((S, S), -1, np.int64)
    yy, xx = np.mgrid[0:S, 0:S]
    for dy in range(-r, r + 1):             # row-major over the window: a later tap wins only if strictly larger
        for dx in range(-r, r + 1):
            y, x = yy + dy, xx + dx
            ok = (y >= 0) & (y < S) & (x >= 0) & (x < S)
            v = np.where(ok, img[np.clip(y, 0, S - 1), np.clip(x, 0, S - 1)], -np.inf)
            win = ok & (v > best)
            best = np.where(win, v, best)
            arg = np.where(win, y * S + x, arg)
    return best, arg


def edges_brute(image_ref, k):
    """compute_edges: maxpool_k(image_ref) - image_ref, float32 like the input"""
    image_ref = np.asarray(image_ref, np.float32)
    return np.stack([maxpool_brute(im, k)[0] - im for im in image_ref]).astype(np.float32)


def edge_edt_brute(image_ref, k, power=0.25):
    """prepare_dist_trans: float32((distance to the nearest pixel with edges > 0) ^ (2 power)), the distance as the float64 sqrt
    of the exact integer square"""
    e = edges_brute(image_ref, k)
    d = np.stack([np.sqrt(edt_sq_brute(x > 0).astype(np.float64)) for x in e])
    return (np.sqrt(d) if power == 0.25 else d ** (2 * power)).astype(np.float32)


def square_boxes(xywh, expansion):
    """PHOSA's make_bbox_square in float64, operation by operation: (B,4) xywh -> (B,4) x, y, s, s"""
    b = np.asarray(xywh, np.float64)
    cx, cy = b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2
    s = np.maximum(b[:, 2], b[:, 3]) * (1 + expansion)
    return np.stack([cx - s / 2, cy - s / 2, s, s], 1)


def roi_intrinsics(squares, crop_centers, crop_size=1200, net_input_size=512, kinect_width=2048):
    """to_original_bbox and compute_K_roi in float64, rounded to float32 at the end: (B,4), (B,2) -> (bbox_orig (B,4), K (B,3,3))"""
    scale = crop_size / float(net_input_size)
    b = np.asarray(squares, np.float64) * scale
    b[:, :2] += np.asarray(crop_centers, np.float64) - crop_size / 2.0
    fx, fy = 979.7844 / kinect_width, 979.840 / kinect_width
    cx, cy = 1018.952 / kinect_width, 779.486 / kinect_width
    K = np.zeros((len(b), 3, 3), np.float64)
    K[:, 0, 0] = fx * kinect_width / b[:, 2]
    K[:, 1, 1] = fy * kinect_width / b[:, 2]
    K[:, 0, 2] = (cx * kinect_width - b[:, 0]) / b[:, 2]
    K[:, 1, 2] = (cy * kinect_width - b[:, 1]) / b[:, 2]
    K[:, 2, 2] = 1
    return b, K.astype(np.float32)


def crop_values(mask, square, S):
    """the bilinear crop of crop_and_resize in float64, before its threshold: (H,W) mask, box x, y, s, s -> (S,S) values sampled
    at x + (i + 0.5) s / S - 0.5, zeros outside the image"""
    m = np.asarray(mask, np.float64)
    H, W = m.shape
    x0, y0 = float(square[0]), float(square[1])
    x1, y1 = x0 + float(square[2]), y0 + float(square[3])
    i = np.arange(S, dtype=np.float64)
    px = x0 + (i + 0.5) * (x1 - x0) / S - 0.5
    py = y0 + (i + 0.5) * (y1 - y0) / S - 0.5
    fx, fy = np.floor(px), np.floor(py)
    wx1, wy1 = px - fx, py - fy
    pad = np.zeros((H + 2, W + 2))
    pad[1:-1, 1:-1] = m
    ix = np.clip(fx.astype(np.int64), -1, W - 1) + 1          # left tap in the padded image; a tap beyond it reads a zero
    iy = np.clip(fy.astype(np.int64), -1, H - 1) + 1
    inx, iny = (fx >= -1) & (fx <= W - 1), (fy >= -1) & (fy <= H - 1)
    out = np.zeros((S, S))
    for ty, wy in ((0, 1 - wy1), (1, wy1)):
        for tx, wx in ((0, 1 - wx1), (1, wx1)):
            out += pad[np.ix_(iy + ty, ix + tx)] * (wy * iny)[:, None] * (wx * inx)[None, :]
    return out


def targets_brute(person, obj, S, expansion=0.3):
    """what SilLossROI.from_masks promises, in float64 numpy: -> image_ref, keep_mask (B,S,S) float32, squares (B,4), valid (B),
    and the smallest |value - 0.5| over every crop value of the valid frames"""
    person, obj = np.asarray(person, np.float32), np.asarray(obj, np.float32)
    B, H, W = obj.shape
    image_ref, keep = np.zeros((B, S, S), np.float32), np.zeros((B, S, S), np.float32)
    squares, valid, margin = np.zeros((B, 4)), np.zeros(B, np.int32), np.inf
    for b in range(B):
        ys, xs = np.nonzero(obj[b] > 0.5)
        if ys.size == 0:
            squares[b] = (0, 0, max(H, W), max(H, W))
            continue
        box = np.array([[xs.min(), ys.min(), xs.max() + 1 - xs.min(), ys.max() + 1 - ys.min()]], np.float64)
        squares[b] = square_boxes(box, expansion)[0]
        vo, vp = crop_values(obj[b], squares[b], S), crop_values(person[b], squares[b], S)
        margin = min(margin, np.abs(vo - 0.5).min(), np.abs(vp - 0.5).min())
        fore, ps = vo >= 0.5, vp >= 0.5
        image_ref[b], keep[b], valid[b] = fore, fore | ~ps, 1
    return image_ref, keep, squares, valid, margin


# ---- the fixture pins them ---------------------------------------------------------------------------------------------
def test_edges_and_distance_transform_reproduce_the_reference():
    g = golden("sil_project.npz")
    image_ref = g["image_ref"]
    assert image_ref.shape == (3, 64, 64) and set(np.unique(image_ref)) == {0.0, 1.0}
    edges = edges_brute(image_ref, 7)
    assert edges.dtype == np.float32 and np.array_equal(edges, g["ref_edges"])
    edt = edge_edt_brute(image_ref, 7)
    assert edt.dtype == g["edt_ref_edge"].dtype == np.float32
    assert np.array_equal(edt.view(np.uint32), g["edt_ref_edge"].view(np.uint32))
    assert (g["ref_edges"] > 0).any(axis=(1, 2)).all() and float(g["edt_ref_edge"].max()) > 2       # every frame has an outline


def test_box_arithmetic_reproduces_the_reference():
    g = golden("sil_project.npz")
    sq = square_boxes(g["boxes_xywh"], 0.3)
    assert np.array_equal(sq.view(np.uint64), g["squares"].view(np.uint64))
    orig, K = roi_intrinsics(sq, g["crop_centers"])
    assert np.array_equal(orig.view(np.uint64), g["bbox_orig"].view(np.uint64))
    assert K.dtype == np.float32 and np.array_equal(K.view(np.uint32), g["K"].view(np.uint32))


def test_brute_force_distance_on_known_images():
    """the brute force itself, on images whose transform is known in closed form"""
    f = np.zeros((5, 7), np.uint8)
    f[0, 0] = 1
    yy, xx = np.mgrid[0:5, 0:7]
    assert np.array_equal(edt_sq_brute(f), yy * yy + xx * xx)
    assert np.array_equal(edt_sq_brute(np.ones((4, 3))), np.zeros((4, 3), np.int64))
    assert np.array_equal(edt_sq_brute(np.zeros((4, 9))), np.full((4, 9), 162))
    f = np.zeros((6, 6), np.uint8)
    f[:, 2] = 1
    assert np.array_equal(edt_sq_brute(f), (np.mgrid[0:6, 0:6][1] - 2) ** 2)


def test_sentinel_and_tiles_without_gpu():
    """the library's documented constants: the sentinel of an image without features is the restatement's, the tile sizes the
    GPU case table is built around, and the workspace sizes refuse what the kernels refuse"""
    from chore_amd import _lib
    from chore_amd.preprocess.edt import edt_sentinel, edt_tiles
    assert edt_tiles() == (64, 256, 4096)
    for H, W in ((1, 1), (4, 9), (256, 37)):
        assert edt_sentinel(H, W) == int(edt_sq_brute(np.zeros((H, W)))[0, 0]) > (H - 1) ** 2 + (W - 1) ** 2
    assert _lib.lib.chore_edt_workspace_bytes(2, 63, 65) >= 2 * 63 * 65 * 4
    assert _lib.lib.chore_edt_workspace_bytes(1, 4097, 8) == 0 and _lib.lib.chore_edt_workspace_bytes(1, 8, 4097) == 0
    assert _lib.lib.chore_sil_edge_edt_workspace_bytes(3, 64) >= 3 * 64 * 64 * 9
    assert _lib.lib.chore_sil_edge_workspace_bytes(2, 65) >= 2 * 17 * 4 and _lib.lib.chore_sil_targets_workspace_bytes(3) >= 48


def test_crop_restatement_matches_the_host_constructor_away_from_the_threshold():
    """crop_values against crop_and_resize's grid_sample (float32) on a smooth image: the values agree to float32 round-off, so
    the restatement samples where the constructor samples"""
    import torch
    import torch.nn.functional as F
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:40, 0:52]
    img = (np.sin(xx * 0.31) * np.cos(yy * 0.23) * 0.5 + 0.5 + rs.uniform(0, 0.05, (40, 52))).astype(np.float32)
    for sq, S in (((3.25, 5.5, 20.0, 20.0), 16), ((-6.0, 30.0, 31.5, 31.5), 9), ((44.0, -3.0, 12.0, 12.0), 7)):
        want = crop_values(img, sq, S)
        x0, y0, x1, y1 = sq[0], sq[1], sq[0] + sq[2], sq[1] + sq[3]
        xs = x0 + (torch.arange(S, dtype=torch.float32) + 0.5) * (x1 - x0) / S - 0.5
        ys = y0 + (torch.arange(S, dtype=torch.float32) + 0.5) * (y1 - y0) / S - 0.5
        grid = torch.stack(torch.meshgrid(2 * ys / 39 - 1, 2 * xs / 51 - 1, indexing="ij")[::-1], -1)[None]
        got = F.grid_sample(torch.from_numpy(img)[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]
        assert np.abs(got.numpy() - want).max() < 2e-5, (sq, np.abs(got.numpy() - want).max())
