"""float64 references of the fitting-step and evaluation operators (csrc/smpl_lbs.hip, fit_terms.hip, fit_step.hip, so3.hip,
contact.hip, eval_metrics.hip), for tests/test_gpu_fit_kernels.py.  Plain torch / numpy on the CPU, autograd for the gradients;
no kernel of the library is called here.  Each function restates the operation as the headers of those files describe it:
  lbs              SMPL-H linear blend skinning: Rodrigues through the quaternion path with angle = ||theta + 1e-8||, shape and pose
                   blend, joints, kinematic chain, skinning (pinned against tests/golden/smpl_lbs.npz by test_fit_coverage_table.py)
  smpl_terms       body prior, hand prior with the batch-axis quirk (summed over frames and hands, mean over the 45 columns),
                   pose-init, SMPL depth, keypoint reprojection -- the tensor expressions of recon/recon_fit_base.py
  point_terms, obj_transform, obj_terms       likewise
  contact          oracle.contact.contact_loss on float64 inputs, and which points sit on a nearest-neighbour tie
  adam_step, stop_rule, weighted_sum          the formulas of the header of fit_step.hip (the last two in fp32 numpy: bit for bit)
  chamfer, procrustes, so3_project            brute force / numpy.linalg.svd; the so3 gradient by central differences
`dtype` is torch.float64 everywhere; lbs also runs in torch.float32, which is the reference implementation's own arithmetic."""
import numpy as np
import torch

F64 = torch.float64


def t64(a, grad=False):
    return torch.as_tensor(np.asarray(a), dtype=F64).clone().requires_grad_(grad)


# ================================================================================================ SMPL-H LBS
def rodrigues(theta):
    """(...,3) axis-angle -> (...,3,3) through the unit quaternion, renormalised"""
    angle = torch.linalg.norm(theta + 1e-8, dim=-1, keepdim=True)
    axis = theta / angle
    half = angle * 0.5
    quat = torch.cat([torch.cos(half), torch.sin(half) * axis], -1)
    quat = quat / torch.linalg.norm(quat, dim=-1, keepdim=True)
    w, x, y, z = quat[..., 0], quat[..., 1], quat[..., 2], quat[..., 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    R = torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                     2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                     2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], -1)
    return R.reshape(theta.shape[:-1] + (3, 3))


def lbs_model(model, dtype=F64):
    """the arrays of synth.synth_smplh_model as tensors of `dtype`"""
    m = {k: torch.as_tensor(np.asarray(model[k]), dtype=dtype) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    m["parents"] = [int(p) for p in model["parents"]]
    return m


def lbs(m, pose, betas, trans, offsets=None, scale=1.0):
    """pose (B,3J), betas (B,nb), trans (B,3), offsets (B,V,3) or None -> verts (B,V,3), joints (B,J,3), v_posed, naked"""
    B, parents = pose.shape[0], m["parents"]
    J, V = len(parents), m["v_template"].shape[0]
    R = rodrigues(pose.reshape(B, J, 3))
    pose_map = (R[:, 1:] - torch.eye(3, dtype=pose.dtype)).reshape(B, (J - 1) * 9)
    v_shaped = m["v_template"][None] + torch.einsum("vkn,bn->bvk", m["shapedirs"], betas)
    jl = torch.einsum("jv,bvk->bjk", m["J_regressor"], v_shaped)
    naked = v_shaped + (pose_map @ m["posedirs"].reshape(V * 3, -1).T).reshape(B, V, 3)
    v_posed = naked if offsets is None else naked + offsets
    Rg, tg = [R[:, 0]], [jl[:, 0]]
    for i in range(1, J):
        p = parents[i]
        Rg.append(Rg[p] @ R[:, i])
        tg.append((Rg[p] @ (jl[:, i] - jl[:, p]).unsqueeze(-1)).squeeze(-1) + tg[p])
    Rg, tg = torch.stack(Rg, 1), torch.stack(tg, 1)                       # (B,J,3,3), (B,J,3)
    At = tg - (Rg @ jl.unsqueeze(-1)).squeeze(-1)                         # the rest pose removed
    TR = torch.einsum("vj,bjrc->bvrc", m["weights"], Rg)
    Tt = torch.einsum("vj,bjr->bvr", m["weights"], At)
    verts = (torch.einsum("bvrc,bvc->bvr", TR, v_posed) + Tt) * scale + trans[:, None]
    joints = tg * scale + trans[:, None]
    return verts, joints, v_posed, naked


def lbs_with_grads(m, pose, betas, trans, offsets, scale, g_verts, g_joints, dtype=F64):
    """-> (verts, joints, v_posed, naked, dpose, dbetas, dtrans) as float64 numpy, computed in `dtype`"""
    c = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype)      # noqa: E731
    p, b, t = (c(a).requires_grad_(True) for a in (pose, betas, trans))
    verts, joints, vp, nk = lbs(m, p, b, t, c(offsets), scale)
    loss = 0
    if g_verts is not None:
        loss = loss + (verts * c(g_verts)).sum()
    if g_joints is not None:
        loss = loss + (joints * c(g_joints)).sum()
    loss.backward()
    return tuple(a.detach().double().numpy() for a in (verts, joints, vp, nk, p.grad, b.grad, t.grad))


# ================================================================================================ loss terms (csrc/fit_terms.hip)
def smpl_terms(pose, pose_init, J, kpts, cc, bmean, bprec, hmean, lprec, rprec, cam8):
    """-> [pose prior, hand prior, pose-init, depth, keypoints] float64 scalars (autograd through pose and J); kpts None: no
    keypoint term (0).  cam8 = fx, fy, cx, cy, crop / 2, crop, network input size, z_0."""
    fx, fy, cx, cy, half_crop, crop, net_in, z0 = cam8
    t2 = (pose[:, 3:66] - bmean) @ bprec
    p_pose = (t2 * t2).sum(1).mean()
    th = pose[:, 66:156] - hmean
    lh, rh = th[:, :45] @ lprec, th[:, 45:] @ rprec
    hands = torch.cat([lh, rh], 0)                      # the two hands concatenated along the BATCH axis and summed over it ...
    p_hand = (hands * hands).sum(0).mean()              # ... then the mean of the 45 columns
    pinit = ((pose[:, 3:72] - pose_init) ** 2).sum(-1).mean()
    smplz = ((J[:, 8, 2] - z0) ** 2).mean()
    if kpts is None:
        j2d = torch.zeros((), dtype=pose.dtype)
    else:
        x, y, z = J[:, :25, 0], J[:, :25, 1], J[:, :25, 2]
        px = half_crop + (fx * x / z + cx) - cc[:, 0:1]
        py = half_crop + (fy * y / z + cy) - cc[:, 1:2]
        proj = torch.stack([px, py], -1) * net_in / crop
        j2d = (((proj - kpts[:, :, :2]) ** 2).sum(-1) * kpts[:, :, 2]).mean()
    return [p_pose, p_hand, pinit, smplz, j2d]


def point_terms(df, channel, cmax, logits, labels):
    """-> (mean of the clamped channel, cross entropy summed over the points and averaged over the frames, or None)"""
    clamped = torch.clamp(df[:, channel:channel + 1, :], max=cmax).mean()
    if logits is None:
        return clamped, None
    ce = torch.nn.functional.cross_entropy(logits, labels, reduction="none").sum(-1).mean()
    return clamped, ce


def obj_transform(verts, R, t, s):
    """rotate, translate, THEN scale"""
    return (torch.bmm(verts, R) + t.unsqueeze(1)) * s.unsqueeze(1).unsqueeze(1)


def obj_terms(obj, centers, obj_s, smpl_center, scale0):
    """-> (scale, ocent, the bracket (B,3))"""
    scale = ((obj_s - scale0) ** 2).mean()
    diff = obj.mean(1) - (smpl_center + centers[:, 3:].mean(-1))
    return scale, (diff ** 2).sum(-1).mean(), diff


# ================================================================================================ contact (csrc/contact.hip)
TIE_REL = 1e-6          # nearest and second-nearest squared distance closer than this (relative): fp32 may pick the other one


def contact(hum, obj, df_h, df_o, labels, logits, P, thres, g=1.0):
    """float64: -> (loss, d_hum, d_obj, tie_h (B,Nh) bool, tie_o (B,No) bool, participating points).  A `tie` marks a point
    whose gradient depends on a nearest-neighbour choice that float32 distances may make differently: the point itself and the
    two candidates it could hand its term to."""
    from oracle.contact import contact_loss
    h, o = t64(hum, True), t64(obj, True)
    dfh, dfo, lg, lab = t64(df_h), t64(df_o), t64(logits), torch.as_tensor(np.asarray(labels)).long()
    loss = contact_loss(dfh, dfo, o, h, lg, lab, n_parts=P, thres=thres)
    if loss is None:
        z = np.zeros
        return 0.0, z(h.shape), z(o.shape), z(h.shape[:2], bool), z(o.shape[:2], bool), 0
    (loss * g).backward()
    # the ties, from the same selection rule
    B = h.shape[0]
    tie_h, tie_o, npart = np.zeros(h.shape[:2], bool), np.zeros(o.shape[:2], bool), 0
    part_o = torch.argmax(lg, 1).numpy()
    H, O, lab = h.detach().numpy(), o.detach().numpy(), lab.numpy()
    for b in range(B):
        mh, mo = dfh[b].numpy() < thres, dfo[b].numpy() < thres
        if mh.sum() + mo.sum() == 0:
            continue
        sh = mh if mh.any() else np.ones_like(mh)
        so = mo if mo.any() else np.ones_like(mo)
        for i in range(P):
            hi, oi = np.where(sh & (lab == i))[0], np.where(so & (part_o[b] == i))[0]
            if len(hi) == 0 or len(oi) == 0:
                continue
            npart += len(hi) + len(oi)
            d = ((H[b, hi][:, None] - O[b, oi][None]) ** 2).sum(-1)
            for dd, qi, ci, tq, tc in ((d, hi, oi, tie_h, tie_o), (d.T, oi, hi, tie_o, tie_h)):
                if dd.shape[1] < 2:
                    continue
                two = np.argpartition(dd, 1, axis=1)[:, :2]
                d0, d1 = np.take_along_axis(dd, two, 1).T
                near = np.abs(d1 - d0) < TIE_REL * np.maximum(d0, d1)
                tq[b, qi[near]] = True
                tc[b, ci[two[near]].ravel()] = True
    return float(loss.detach()), h.grad.numpy(), o.grad.numpy(), tie_h, tie_o, npart


# ================================================================================================ the step's tail (csrc/fit_step.hip)
def adam_step(p, g, m, v, t, lr, b1, b2, eps, frozen=False):
    """one update of torch.optim.Adam(capturable=True) in float64 numpy, t = the number of this step (1, 2, ...) -> p, m, v"""
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    step_size = -lr / (1.0 - b1 ** t)
    if not frozen:
        p = p + m / (np.sqrt(v) / (np.sqrt(1.0 - b2 ** t) * step_size) + eps / step_size)
    return p, m, v


def stop_rule(loss, prev, stop, armed, tol):
    """fp32, operation for operation: hit = |prev - loss| / prev < prev * tol -> (prev, stop, loss_out)"""
    f = np.float32
    lv, pv, tol = f(loss), f(prev), f(tol)
    with np.errstate(all="ignore"):
        hit = np.abs(pv - lv) / pv < pv * tol
    new_stop = 1 if (stop or (hit and armed)) else 0
    return (pv if stop else lv), new_stop, lv


def weighted_sum(losses, coeffs, denom):
    """fp32, in dictionary order: s += c * L / denom"""
    f = np.float32
    s = f(0.0)
    for c, l in zip(coeffs, losses):
        s = f(s + f(f(f(c) * f(l)) / f(denom)))
    return s


def weighted_sum_bwd(coeffs, denom, g):
    f = np.float32
    return np.array([f(f(f(g) * f(c)) / f(denom)) for c in coeffs], np.float32)


# ================================================================================================ evaluation (csrc/eval_metrics.hip)
def chamfer(x, y):
    """-> (mean_i min_j |x_i - y_j|, mean_j min_i |x_i - y_j|), Euclidean, float64 brute force"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d2 = np.stack([((x[:, None, k] - y[None, :, k]) ** 2) for k in range(3)], 0).sum(0)
    return float(np.sqrt(d2.min(1)).mean()), float(np.sqrt(d2.min(0)).mean())


def procrustes(S1, S2):
    """the similarity that takes S1 (N,3) closest to S2: -> R (3,3), t (3), scale"""
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    mu1, mu2 = S1.mean(0), S2.mean(0)
    X1, X2 = (S1 - mu1).T, (S2 - mu2).T
    var1 = (X1 ** 2).sum()
    K = X1 @ X2.T
    U, s, Vh = np.linalg.svd(K)
    V = Vh.T
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ V.T))
    R = V @ Z @ U.T
    scale = np.trace(R @ K) / var1
    return R, mu2 - scale * (R @ mu1), scale


# ================================================================================================ SO(3) projection (csrc/so3.hip)
def so3_project(M):
    """(B,3,3) float64 -> R = U diag(1, 1, det(U V^T)) V^T, the singular values, d = det(U V^T)"""
    U, s, Vh = np.linalg.svd(np.asarray(M, np.float64))
    d = np.linalg.det(U @ Vh)
    D = np.tile(np.eye(3), (len(s), 1, 1))
    D[:, 2, 2] = d
    return U @ D @ Vh, s, d


def so3_grad(M, G):
    """d sum(R * G) / d M by fourth-order central differences of so3_project in float64, step 1e-6 sigma_1"""
    M, G = np.asarray(M, np.float64), np.asarray(G, np.float64)
    h = 1e-6 * np.linalg.svd(M, compute_uv=False)[:, 0]
    out = np.zeros_like(M)
    for e in range(9):
        E = np.zeros((1, 3, 3))
        E.flat[e] = 1.0
        f = lambda k: (so3_project(M + k * h[:, None, None] * E)[0] * G).sum((1, 2))     # noqa: E731
        out.reshape(-1, 9)[:, e] = (8.0 * (f(1) - f(-1)) - (f(2) - f(-2))) / (12.0 * h)
    return out


def so3_gaps(s, d):
    """the three denominators sigma_i d_i + sigma_j d_j of the projection's derivative, relative to sigma_1 -> (B,) the smallest"""
    sd = s * np.stack([np.ones_like(d), np.ones_like(d), d], 1)
    return np.minimum(np.minimum(sd[:, 0] + sd[:, 1], sd[:, 0] + sd[:, 2]), sd[:, 1] + sd[:, 2]) / s[:, 0]
