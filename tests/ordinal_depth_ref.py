"""Restatement (test infrastructure) of the ordinal depth term of csrc/ordinal_depth.hip in numpy float64, with a running
bound on what a float32 evaluation in the kernel's operation order can differ by.  The winning face per pixel is GIVEN
(chore_silhouette_fwd's own map, or oracle.silhouette's on the host), so a z-buffer tie never enters a comparison of values.

The term (include/chore_hip.h), per frame, on the S x S grid, in the orientation of image_ref (row r = row S-1-r of the winner map):
  d_o   depth of the winning object face: w = clamp(inv (x, y, 1), 0, 1) / sum, zp = 1 / sum_k w_k / z_k, inv the pixel-space
        inverse of the triangle (tests/render_ref.py states the same rule); there is no object where the winner is -1
  d_h   the occluder depth image, GIVEN (float32 values: an input of the kernel), far where there is no body
  both  winner >= 0 and d_h < far;  O = image_ref > 0.5;  P = not O and keep_mask < 0.5
  A     P & both & d_o < d_h: x = min(d_h - d_o, c), term log1p(exp(x)), coef = d term / d d_o = -sigmoid(x) if d_h - d_o <= c else 0
  B     O & both & d_h < d_o: x = min(d_o - d_h, c), the same with the sign +;   equal depths contribute nothing
  counts  pixels in A, in B, in P & both, in O & both

Error bounds: class E carries a value and a bound on |float32 result - value| through every operation of the kernel's order:
an operation on operands with bounds ea, eb returns the propagated bound (|a| eb + |b| ea + ea eb for a product,
(ea + |a / b| eb) / (|b| - eb) for a quotient, ea + eb for a sum; clamps and min are 1-Lipschitz) plus one rounding,
2^-24 (|result| + propagated).  float32 inputs and small integers are exact.  expf and log1pf add ULP_EXPF / ULP_LOG1PF units
of 2^-23 |result|: the HIP math API documents a maximum error of 1 ulp for both (CUDA's table: 2 and 1); 2 each are budgeted.
"""
import numpy as np

import render_bwd_ref

U = 2.0 ** -24                  # unit round-off of float32
ULP_EXPF = ULP_LOG1PF = 2       # budgeted ulps of the device's expf / log1pf (documented: 1)
C = 2.0                         # PHOSA's clamp
FAR = 100.0


def sum_chain(S):
    """longest addition chain of chore_ordinal_depth_fwd's per-frame sum (include/chore_hip.h): 8 tree levels in a block of 256
    pixels, ceil(blocks / 256) partials per thread, 8 tree levels over the threads"""
    nblk = -(-S * S // 256)
    return 16 + -(-nblk // 256)


class E:
    """value v (float64) and bound e on |float32 evaluation - v|"""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)
        if np.isnan(self.e).any():       # (an infinite bound times a zero value: still no bound)
            self.e = np.where(np.isnan(self.e), np.inf, self.e)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(np.float64(x))

    @staticmethod
    def _r(v, e):                # one rounding on top of the propagated bound
        return E(v, e + U * (np.abs(v) + e))

    def __add__(self, o):
        o = E.of(o)
        return E._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = E.of(o)
        return E._r(self.v - o.v, self.e + o.e)

    def __neg__(self):
        return E(-self.v, self.e)

    def __mul__(self, o):
        o = E.of(o)
        return E._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = E.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            room = np.abs(o.v) - o.e
            e = np.where(room > 0, (self.e + np.abs(v) * o.e) / np.where(room > 0, room, 1.0), np.inf)
        return E._r(v, e)

    def half(self):              # exact in binary floating point
        return E(0.5 * self.v, 0.5 * self.e)

    def clip01(self):
        return E(np.clip(self.v, 0.0, 1.0), self.e)

    def minimum(self, c):
        return E(np.minimum(self.v, c), self.e)

    def exp(self):
        v = np.exp(self.v)
        e = v * np.expm1(self.e)
        return E(v, e + ULP_EXPF * 2 * U * (v + e))

    def log1p(self):             # argument >= 0 here: the derivative is at most 1
        v = np.log1p(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            room = 1.0 + self.v - self.e
            e = np.where(room > 0, self.e / np.where(room > 0, room, 1.0), np.inf)
        return E(v, e + ULP_LOG1PF * 2 * U * (np.abs(v) + e))

    def __getitem__(self, i):
        return E(self.v[i], self.e[i])


def depth_rule(tri, b, fim):
    """for the hit pixels of frame b (rows of the winner map): (yi, xi, fn, w [3 x E], zp E, inv [9 x E], z [3 x E]) -- the values
    are tests/render_bwd_ref.py _winner_terms' in float64 (asserted), the bounds follow the kernel's operations (tri_setup,
    raster_weights)"""
    tri = np.asarray(tri, np.float32).astype(np.float64)
    S = fim.shape[1]
    yi, xi = np.nonzero(fim[b] >= 0)
    fn = fim[b, yi, xi]
    f = tri[b, fn]
    Sf = E(np.float64(S))
    p = [[((E(f[:, v, d]) * Sf + Sf) - 1.0).half() for d in range(2)] for v in range(3)]
    den = (p[2][0] * (p[0][1] - p[1][1]) + p[0][0] * (p[1][1] - p[2][1])) + p[1][0] * (p[2][1] - p[0][1])
    m = [p[1][1] - p[2][1], p[2][0] - p[1][0], p[1][0] * p[2][1] - p[2][0] * p[1][1],
         p[2][1] - p[0][1], p[0][0] - p[2][0], p[2][0] * p[0][1] - p[0][0] * p[2][1],
         p[0][1] - p[1][1], p[1][0] - p[0][0], p[0][0] * p[1][1] - p[1][0] * p[0][1]]
    inv = [mk / den for mk in m]
    xf, yf = E(xi.astype(np.float64)), E(yi.astype(np.float64))
    w = [((inv[3 * k] * xf + inv[3 * k + 1] * yf) + inv[3 * k + 2]).clip01() for k in range(3)]
    ws = (w[0] + w[1]) + w[2]
    w = [wk / ws for wk in w]
    z = [E(f[:, k, 2]) for k in range(3)]
    zp = E(1.0) / ((w[0] / z[0] + w[1] / z[1]) + w[2] / z[2])
    if yi.size:
        want = render_bwd_ref._winner_terms(tri, b, fim, np.float64)
        assert np.array_equal(want[4], zp.v) and all(np.array_equal(a, c.v) for a, c in zip(want[3], w))
    return yi, xi, fn, w, zp, inv, z


def winner_depth(tri, fim, far=FAR, flip=True):
    """(B,S,S) float64 depth of the winners and the bound on a float32 evaluation, far (bound 0) where there is none; flip: in
    the orientation of image_ref"""
    B, S = fim.shape[:2]
    d = np.full((B, S, S), np.float64(np.float32(far)))
    e = np.zeros((B, S, S))
    for b in range(B):
        yi, xi, _, _, zp, _, _ = depth_rule(tri, b, fim)
        d[b, yi, xi], e[b, yi, xi] = zp.v, zp.e
    return (d[:, ::-1].copy(), e[:, ::-1].copy()) if flip else (d, e)


def forward(tri, fim, occ, image_ref, keep_mask, c=C, far=FAR, same=None, d32=None):
    """the term from a given winner map `fim` (B,S,S, rows not flipped), occluder depth and masks (B,S,S, image_ref's
    orientation) -> dict of float64 arrays in image_ref's orientation: d_o, d_err; terms, term_err; coef, coef_err; the bool
    maps case_a, case_b, p_both, o_both, tie (both, labelled, exactly equal depths), beyond (a case whose difference exceeds c);
    counts (B,4) int64; sums (B); abs_sums (B).
    The three yes / no questions of a pixel (d_o < d_h?  equal?  difference <= c?) have no tolerance: a float64 depth within
    round-off of d_h answers them differently from any float32 evaluation, and an edge-on face -- whose depth is ill-conditioned,
    bound 1e-3 and more -- makes that a common event.  So they are answered on GIVEN float32 depths where there are any:
      d32   (B,S,S) float32, image_ref's orientation: the winners' depth as the merged depth rule gives it in float32
            (chore_sil_depth's image, pinned bit for bit to chore_render_fwd's; on the host tests/render_bwd_ref.py in float32),
            compared with d_h by the kernel's own float32 subtraction.  d_o, every term and every coef stay float64 values of
            the winner map, with bounds that cover the float32 evaluation; depth_ratio = the largest |d32 - d_o| / d_err.
            Also returned then, with the suffix _g: terms, coef, sums and their bounds evaluated ON d32 (see below).
      same  (B,S,S) bool, without d32: pixels where the occluder's winner is GIVEN to be the very triangle that wins for the
            object (a scene built that way): equal depths."""
    c32 = np.float32(c)
    c = np.float64(c32)
    farf = np.float64(np.float32(far))
    occ32 = np.asarray(occ, np.float32)
    occ = occ32.astype(np.float64)
    O = np.asarray(image_ref) > 0.5
    P = ~O & (np.asarray(keep_mask) < 0.5)
    d_o, d_err = winner_depth(tri, fim, far, flip=True)
    both = (fim[:, ::-1] >= 0) & (occ < farf)
    diff = E(np.where(P, occ - d_o, d_o - occ), d_err)
    diff = E._r(diff.v, diff.e)                      # the subtraction's rounding
    if same is not None:
        diff = E(np.where(same, 0.0, diff.v), np.where(same, 0.0, diff.e))
    out = {"d_o": d_o, "d_err": d_err}
    if d32 is not None:
        d32 = np.asarray(d32, np.float32)
        diff32 = np.where(P, occ32 - d32, d32 - occ32)
        assert diff32.dtype == np.float32
        pos, zero, within = diff32 > 0, diff32 == 0, diff32 <= c32
        hit = fim[:, ::-1] >= 0
        with np.errstate(all="ignore"):
            out["depth_ratio"] = float((np.abs(d32.astype(np.float64) - d_o)[hit] / d_err[hit]).max()) if hit.any() else 0.0
    else:
        pos, zero, within = diff.v > 0, diff.v == 0, diff.v <= c
    lab = both & (P | O)
    viol = lab & pos
    tie = lab & zero
    with np.errstate(all="ignore"):
        x = diff.minimum(c)
        term = x.exp().log1p()
        sg = E(1.0) / (E(1.0) + (-x).exp())
    passes = viol & within
    out.update({"tie": tie, "case_a": viol & P, "case_b": viol & O, "p_both": both & P, "o_both": both & O, "beyond": viol & ~within})
    out["terms"] = np.where(viol, term.v, 0.0)
    out["term_err"] = np.where(viol, term.e, 0.0)
    out["coef"] = np.where(passes, np.where(P, -sg.v, sg.v), 0.0)
    out["coef_err"] = np.where(passes, sg.e, 0.0)
    out["counts"] = np.stack([out[k].sum((1, 2)) for k in ("case_a", "case_b", "p_both", "o_both")], 1).astype(np.int64)
    out["sums"] = out["terms"].sum((1, 2))
    out["abs_sums"] = np.abs(out["terms"]).sum((1, 2))
    out["term_err_sums"] = out["term_err"].sum((1, 2))
    if d32 is not None:
        # the second stage alone: the same expressions on the GIVEN float32 depths (exact inputs) -- one subtraction, expf, log1pf,
        # and for coef one more expf, an addition and a division; no depth rule, so no ill-conditioned face loosens these bounds
        d64 = d32.astype(np.float64)
        dg = E._r(np.where(P, occ - d64, d64 - occ), 0.0)
        xg = dg.minimum(c)
        tg = xg.exp().log1p()
        sgg = E(1.0) / (E(1.0) + (-xg).exp())
        out["terms_g"], out["term_err_g"] = np.where(viol, tg.v, 0.0), np.where(viol, tg.e, 0.0)
        out["coef_g"], out["coef_err_g"] = np.where(passes, np.where(P, -sgg.v, sgg.v), 0.0), np.where(passes, sgg.e, 0.0)
        out["sums_g"], out["abs_sums_g"] = out["terms_g"].sum((1, 2)), np.abs(out["terms_g"]).sum((1, 2))
        out["term_err_sums_g"] = out["term_err_g"].sum((1, 2))
    return out


def backward(tri, fim, coef, g):
    """grad_tri (B,F,3,3) float64 and the bound on the kernel's float32 result, from GIVEN coef (B,S,S, image_ref's orientation;
    float32 values, an input of chore_ordinal_depth_bwd) and g (B): the depth rule of chore_render_bwd (tests/render_bwd_ref.py
    depth_bwd, asserted equal) applied to the per-pixel gradient coef * g (one float32 product).  A face's three sums are added
    in float32 along a chain of at most (pixels it won) + 9 additions."""
    tri32 = np.asarray(tri, np.float32)
    B, Fn = tri32.shape[:2]
    S = fim.shape[1]
    coef = np.asarray(coef, np.float32).astype(np.float64)[:, ::-1]          # rows of the winner map
    g = np.asarray(g, np.float32).astype(np.float64)
    val, err = np.zeros((B, Fn, 3, 3)), np.zeros((B, Fn, 3, 3))
    gd = np.zeros((B, S, S))
    for b in range(B):
        yi, xi, fn, w, zp, inv, z = depth_rule(tri32, b, fim)
        if yi.size == 0:
            continue
        gp = E(coef[b, yi, xi]) * E(g[b])
        gd[b, yi, xi] = coef[b, yi, xi] * g[b]
        a = gp * (zp * zp)
        won = np.bincount(fn, minlength=Fn).astype(np.float64)
        first = np.full(Fn, -1)
        first[fn[::-1]] = np.arange(yi.size)[::-1]                           # one pixel of every winning face (its setup values)
        faces = np.nonzero(won)[0]
        k0 = first[faces]
        tmp = []
        for l in range(2):
            t = E(np.zeros(faces.size))
            for k in range(3):
                t = t + (-inv[3 * k + l][k0]) / z[k][k0]
            tmp.append(t)
        n = won[faces] + 9
        for k in range(3):
            ak = a * w[k]
            sv, se, sa = np.zeros(Fn), np.zeros(Fn), np.zeros(Fn)
            np.add.at(sv, fn, ak.v)
            np.add.at(se, fn, ak.e)
            np.add.at(sa, fn, np.abs(ak.v) + ak.e)
            A = E(sv[faces], se[faces] + n * U / (1 - n * U) * sa[faces])
            zk = z[k][k0]
            zero = (A.v == 0) & (A.e == 0)                   # the kernel writes 0 for a sum that is exactly 0
            with np.errstate(all="ignore"):
                gz = A / (zk * zk)
                val[b, faces, k, 2], err[b, faces, k, 2] = np.where(zero, 0.0, gz.v), np.where(zero, 0.0, gz.e)
                for l in range(2):
                    gx = ((-A) * tmp[l] * float(S)).half()
                    val[b, faces, k, l], err[b, faces, k, l] = np.where(zero, 0.0, gx.v), np.where(zero, 0.0, gx.e)
    want = render_bwd_ref.depth_bwd(tri32, fim, gd, np.float64)
    scale = max(float(np.abs(want).max()), 1e-300)
    assert np.abs(want - val).max() <= 1e-9 * scale, "the two restatements of the depth rule differ"
    return val, err


# ---- scenes of the host test (the GPU test builds its own through SilLossROI) ----------------------------------------------
BOX_FACES = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 4, 5], [0, 5, 1], [1, 5, 6], [1, 6, 2], [2, 6, 7], [2, 7, 3],
                      [3, 7, 4], [3, 4, 0]], np.int64)


def box_verts(half=(0.3, 0.2, 0.15)):
    s = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64)
    return (s * np.asarray(half)).astype(np.float32)


def rot_xyz(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def pinhole_tri(verts, faces, focal=1.6):
    """camera-space vertices (V,3) float32 and faces (F,3) -> (2F,3,3) float32 projected triangles [x f / z, y f / z, z], both
    windings (faces, then the reversed corners)"""
    v = np.asarray(verts, np.float32)
    p = np.stack([v[:, 0] * np.float32(focal) / v[:, 2], v[:, 1] * np.float32(focal) / v[:, 2], v[:, 2]], 1).astype(np.float32)
    f = np.asarray(faces, np.int64)
    return p[np.concatenate([f, f[:, ::-1]])]


def block_masks(B, S, seed):
    """image_ref and keep_mask (B,S,S) float32 in 8 x 8 blocks: a third object, a third person, a third free; disjoint"""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 3, (B, -(-S // 8), -(-S // 8)))
    lab = np.repeat(np.repeat(lab, 8, 1), 8, 2)[:, :S, :S]
    return (lab == 1).astype(np.float32), (lab != 2).astype(np.float32)
