"""The point query in float64 on the CPU: what tests/test_gpu_query_kernels.py holds every query kernel against.  numpy only; no
import of chore_amd and no call into the library.  A restatement of the reference's
  model/camera.py   KinectColorCamera.project_screen / normalize   pinhole projection, crop shift, normalisation to [-1, 1]
  model/geometry.py index                                          bilinear sample, zero padding, aligned corners
  model/chore.py    CHORE.query / decode                           in-image test, z_feat, the 323-vector, the four heads, OUT_DIST
  recon/generator.py Generator.approx_surface                      one projection step of Alg. 1
and of their derivatives, written out by hand (no autograd): tests/test_query_coverage_table.py ties them to the reference's own
results in tests/golden/query_full.npz and query_train_grads.npz.

Layouts are those of include/chore_hip.h: maps NHWC, points (B, N, 3), outputs (B, C, N), the training quantities point-major with
P = B * N rows: X [P][328], H [3][4][P][128], dZ [3][4][P][128], dX [P][328]; heads in the order df, parts, pca, centers.

Every function takes `dt`: float64 is the reference, float32 evaluates THE SAME formulas in single precision, which gives the error a
correct float32 implementation may have (the floor of a bound, see query_kernel_cases.FLOORS).  Maps arrive as copies of the values
the kernel reads (for bf16 and fp16 maps: the rounded ones); the camera constants are the float32 values the library is handed.

Besides the results, forward() returns per point what decides whether a float32 implementation may legitimately differ:
  margin  smallest |pre-activation| over the 4 x 384 hidden units (a ReLU that may flip), the smaller of two float64 evaluations: at
          the exact sample coordinates and at the coordinates float32 rounds them to
  line    distance of the sample coordinates of both maps from the nearest texel line, in texels (a tap set that may change)
  border  distance of the normalised coordinates from +-1 (an in-image test that may flip)
and surface_step() returns |df - thr| (a clamp that may flip)."""
import numpy as np

OUT_DIST = 5.0
FEAT_C, TMPX_C, XDIM, KPAD, HID = 256, 64, 323, 328, 128
HEADS = ("df", "part_predictor", "pca_predictor", "center_predictor")      # the order of the staging planes and of the live mask's bits
OUT_NAMES = ("df", "parts", "pca", "centers")
OUT_DIM = (2, 14, 9, 6)
LAYERS = (0, 2, 4, 6)
# model/camera.py, KinectColorCamera.__init__: normalised intrinsics times the image size, and the crop
_F32 = np.float32
CAM6 = tuple(float(_F32(v)) for v in ((979.7844 / 2048.) * 2048, (979.840 / 2048.) * 2048, (1018.952 / 2048.) * 2048,
                                      (779.486 / 2048.) * 2048, 1200 / 2, 1200))


def project(points, crop_center, dt=np.float64):
    """points (B, N, 3), crop_center (B, 2) -> nx, ny (B, N)"""
    fx, fy, cx, cy, half, crop = (dt(v) for v in CAM6)
    p, cc = np.asarray(points, dt), np.asarray(crop_center, dt)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    px = half + (fx * x / z + cx) - cc[:, 0:1]
    py = half + (fy * y / z + cy) - cc[:, 1:2]
    return dt(2) * px / crop - dt(1), dt(2) * py / crop - dt(1)


def sample(m, nx, ny):
    """m (B, H, W, C), nx, ny (B, N) -> dict: val (B, N, C), its derivatives dnx, dny with respect to nx and ny, the flat texel index
    idx (4, B, N) (-1: outside the map) and weight w (4, B, N) of the taps nw, ne, sw, se, and line (B, N)"""
    dt = m.dtype.type
    B, H, W, C = m.shape
    sx, sy = dt((W - 1) / 2), dt((H - 1) / 2)
    ix, iy = (nx + dt(1)) * sx, (ny + dt(1)) * sy
    x0f, y0f = np.floor(ix), np.floor(iy)
    w, n = ix - x0f, iy - y0f
    e, s = dt(1) - w, dt(1) - n
    x0 = np.clip(x0f, -4, W + 4).astype(np.int64)
    y0 = np.clip(y0f, -4, H + 4).astype(np.int64)
    bi = np.arange(B)[:, None]
    taps, idx = [], []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = x0 + dx, y0 + dy
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        taps.append(m[bi, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * ok[..., None].astype(dt))
        idx.append(np.where(ok, yy * W + xx, -1))
    nw, ne, sw, se = taps
    wt = np.stack([e * s, w * s, e * n, w * n])
    val = nw * wt[0][..., None] + ne * wt[1][..., None] + sw * wt[2][..., None] + se * wt[3][..., None]
    dix = (ne - nw) * s[..., None] + (se - sw) * n[..., None]
    diy = (sw - nw) * e[..., None] + (se - ne) * w[..., None]
    line = np.minimum(np.minimum(w, e), np.minimum(n, s))
    return dict(val=val, dnx=dix * sx, dny=diy * sy, idx=np.stack(idx), w=wt, line=line)


def head_weights(sd, dt=np.float64):
    """state dict '<head>.<0|2|4|6>.<weight|bias>' (weights (out, in) or (out, in, 1)) -> [head][layer] (W (out, in), b)"""
    return [[(np.asarray(sd["%s.%d.weight" % (h, l)], dt).reshape(-1, XDIM if l == 0 else HID), np.asarray(sd["%s.%d.bias" % (h, l)], dt))
             for l in LAYERS] for h in HEADS]


def forward(points, crop_center, feat, tmpx, sd, dt=np.float64):
    """-> dict: df, parts, pca, centers (B, C, N) (df with OUT_DIST outside the image), in_img (B, N), X (P, 328), H [3][4] of (P, 128),
    raw [4] of (P, C) head outputs before the fill, margin, line, border (P,), X32 (features_f32's X; float64 only) and what backward()
    needs"""
    B, N = np.asarray(points).shape[:2]
    P = B * N
    p = np.asarray(points, dt)
    nx, ny = project(points, crop_center, dt)
    in_img = (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1)
    sf, st = sample(np.asarray(feat, dt), nx, ny), sample(np.asarray(tmpx, dt), nx, ny)
    X = np.zeros((P, KPAD), dt)
    X[:, :FEAT_C] = sf["val"].reshape(P, FEAT_C)
    X[:, FEAT_C:FEAT_C + 2] = p[..., :2].reshape(P, 2)
    X[:, FEAT_C + 2] = (p[..., 2] - dt(2.2)).reshape(P)
    X[:, FEAT_C + 3:XDIM] = st["val"].reshape(P, TMPX_C)
    Wb = head_weights(sd, dt)
    H, raw, margin = [[None] * 4 for _ in range(3)], [], np.full(P, np.inf)
    # the margin also at the sample coordinates as float32 rounds them (features_f32, the X every kernel is held to bit for bit):
    # the rounding of a coordinate moves X by up to 1e-5 on these maps, more than the margin's threshold, and a kernel's ReLU decides
    # on the X it has
    X32 = features_f32(points, crop_center, feat, tmpx)[0] if dt is np.float64 else None
    starts = [X[:, :XDIM]] + ([X32[:, :XDIM].astype(dt)] if X32 is not None else [])
    for h in range(4):
        for i, a in enumerate(starts):
            for l in range(3):
                pre = a @ Wb[h][l][0].T + Wb[h][l][1]
                margin = np.minimum(margin, np.abs(pre).min(1))
                a = np.maximum(pre, dt(0))
                if i == 0:
                    H[l][h] = a
            if i == 0:
                raw.append(a @ Wb[h][3][0].T + Wb[h][3][1])
    out = {OUT_NAMES[h]: np.ascontiguousarray(raw[h].reshape(B, N, OUT_DIM[h]).transpose(0, 2, 1)) for h in range(4)}
    out["df"] = np.where(in_img[:, None, :], out["df"], dt(OUT_DIST))
    border = np.minimum(np.abs(np.abs(nx) - 1), np.abs(np.abs(ny) - 1)).reshape(P)
    out.update(in_img=in_img, X=X, X32=X32, H=H, raw=raw, margin=margin, line=np.minimum(sf["line"], st["line"]).reshape(P), border=border,
               nx=nx, ny=ny, points=p, Wb=Wb, sf=sf, st=st, B=B, N=N, dt=dt)
    return out


def backward(f, grads):
    """f: forward()'s result; grads: [4] of (B, C, N) upstream gradients of df, parts, pca, centers (heads' order), None = absent.
    The gradient of df does not pass the OUT_DIST fill.  -> dZ [3][4] of (P, 128), dX (P, 328), dpoints (B, N, 3)"""
    dt, B, N = f["dt"], f["B"], f["N"]
    P = B * N
    dZ, dX = [[np.zeros((P, HID), dt) for _ in range(4)] for _ in range(3)], np.zeros((P, KPAD), dt)
    for h in range(4):
        if grads[h] is None:
            continue
        g = np.asarray(grads[h], dt).reshape(B, OUT_DIM[h], N).transpose(0, 2, 1).reshape(P, OUT_DIM[h])
        if h == 0:
            g = g * f["in_img"].reshape(P, 1).astype(dt)
        d = g
        for l in (2, 1, 0):
            d = (d @ f["Wb"][h][l + 1][0]) * (f["H"][l][h] > 0).astype(dt)
            dZ[l][h] = d
        dX[:, :XDIM] += d @ f["Wb"][h][0][0]
    fx, fy, _, _, _, crop = (dt(v) for v in CAM6)
    dxf, dxt = dX[:, :FEAT_C].reshape(B, N, FEAT_C), dX[:, FEAT_C + 3:XDIM].reshape(B, N, TMPX_C)
    gnx = (dxf * f["sf"]["dnx"]).sum(-1) + (dxt * f["st"]["dnx"]).sum(-1)
    gny = (dxf * f["sf"]["dny"]).sum(-1) + (dxt * f["st"]["dny"]).sum(-1)
    gpx, gpy = gnx * (dt(2) / crop), gny * (dt(2) / crop)
    x, y, z = (f["points"][..., i] for i in range(3))
    dz3 = dX[:, FEAT_C:FEAT_C + 3].reshape(B, N, 3)
    dp = np.stack([dz3[..., 0] + gpx * fx / z, dz3[..., 1] + gpy * fy / z,
                   dz3[..., 2] - (gpx * fx * x + gpy * fy * y) / (z * z)], -1)
    return dict(dZ=dZ, dX=dX, dpoints=dp)


def surface_step(f, k, thr):
    """out = p - normalize(grad) * min(df[:, k], thr), grad the gradient of sum(clamp(df[:, k], max = thr)): 1 where df <= thr.
    -> out (B, N, 3), clamp (P,): |df - thr|"""
    dt, B, N = f["dt"], f["B"], f["N"]
    dfk = f["df"][:, k]                                            # (B, N), OUT_DIST outside the image
    g = np.zeros((B, 2, N), dt)
    g[:, k] = (dfk <= dt(thr)).astype(dt)
    grad = backward(f, [g, None, None, None])["dpoints"]
    den = np.maximum(np.sqrt((grad * grad).sum(-1, keepdims=True)), dt(1e-12))
    out = f["points"] - grad / den * np.minimum(dfk, dt(thr))[..., None]
    return out, np.abs(dfk - dt(thr)).reshape(B * N)


def param_grads(f, back, grads):
    """the gradients of the 32 head parameters from the staged quantities, as chore_heads_wgrad forms them: dW_l = dZ_l^T H_(l-1),
    db_l = column sums of dZ_l, the output layer from the upstream gradient (df: zeroed outside the image)"""
    dt, B, N = f["dt"], f["B"], f["N"]
    P, out = B * N, {}
    for h in range(4):
        if grads[h] is None:
            continue
        g = np.asarray(grads[h], dt).reshape(B, OUT_DIM[h], N).transpose(0, 2, 1).reshape(P, OUT_DIM[h])
        if h == 0:
            g = g * f["in_img"].reshape(P, 1).astype(dt)
        acts = [f["X"][:, :XDIM]] + [f["H"][l][h] for l in range(3)]
        for l, d in enumerate([back["dZ"][0][h], back["dZ"][1][h], back["dZ"][2][h], g]):
            out["%s.%d.weight" % (HEADS[h], LAYERS[l])] = d.T @ acts[l]
            out["%s.%d.bias" % (HEADS[h], LAYERS[l])] = d.sum(0)
    return out


def scatter_map(s, d, HW):
    """the gradient of one map from dX: every tap receives its weight times the channel's gradient.  s a sample() result, d (B, N, C)
    the map's channels of dX, HW the number of texels -> (B, HW, C)"""
    B, N, C = d.shape
    out = np.zeros((B, HW, C), d.dtype)
    for k in range(4):
        for b in range(B):
            ok = s["idx"][k][b] >= 0
            np.add.at(out[b], s["idx"][k][b][ok], d[b][ok] * s["w"][k][b][ok][:, None])
    return out


# ---------------------------------------------------------------------------------------------------- float32, operation by operation
def _fma(a, b, c):
    """float32 fused multiply-add: the product of two float32 values is exact in float64, and so is the sum's rounding to within the
    double rounding that a 53-bit intermediate of a 24-bit product cannot show"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(_F32)


def features_f32(points, crop_center, feat, tmpx):
    """X (P, 328) and in_img (B, N) as a float32 implementation computes them that follows the reference operation by operation: the
    projection without contraction, ATen's grid_sampler weights and its chain fma(se, w n, fma(sw, e n, fma(ne, w s, nw (e s)))).
    Every operation is correctly rounded, so a kernel that keeps this order agrees bit for bit"""
    fx, fy, cx, cy, half, crop = (_F32(v) for v in CAM6)
    p, cc = np.asarray(points, _F32), np.asarray(crop_center, _F32)
    B, N = p.shape[:2]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    px = (half + ((fx * x) / z + cx)) - cc[:, 0:1]
    py = (half + ((fy * y) / z + cy)) - cc[:, 1:2]
    nx, ny = (_F32(2) * px) / crop - _F32(1), (_F32(2) * py) / crop - _F32(1)
    in_img = (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1)
    X = np.zeros((B * N, KPAD), _F32)

    def index(m):
        m = np.asarray(m, _F32)
        _, H, W, C = m.shape
        ix, iy = (nx + _F32(1)) * _F32((W - 1) / 2), (ny + _F32(1)) * _F32((H - 1) / 2)
        x0f, y0f = np.floor(ix), np.floor(iy)
        w, n = ix - x0f, iy - y0f
        e, s = _F32(1) - w, _F32(1) - n
        x0, y0 = np.clip(x0f, -4, W + 4).astype(np.int64), np.clip(y0f, -4, H + 4).astype(np.int64)
        bi, acc = np.arange(B)[:, None], None
        for (dy, dx), wk in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (e * s, w * s, e * n, w * n)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = m[bi, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * ok[..., None].astype(_F32)
            acc = v * wk[..., None] if acc is None else _fma(v, np.broadcast_to(wk[..., None], v.shape), acc)
        return acc.reshape(B * N, C)
    X[:, :FEAT_C] = index(feat)
    X[:, FEAT_C:FEAT_C + 2] = p[..., :2].reshape(-1, 2)
    X[:, FEAT_C + 2] = (z - _F32(2.2)).reshape(-1)
    X[:, FEAT_C + 3:XDIM] = index(tmpx)
    return X, in_img
