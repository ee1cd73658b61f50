"""The case matrix, the inputs and the coverage table of tests/test_gpu_fit_kernels.py (no GPU needed to import this).

A case is a dict with an `id`; CASES maps a family (one GPU test each) to its cases.  The shapes were chosen by reading the
kernels, around the constants below: every one is the smallest at which the kernel it reaches can still go wrong -- one below,
equal to and one above a block or tile, a last group with fewer frames than FB, more elements than one pass of a capped grid.
COVERAGE has one row per entry point of chore_amd/_lib.py of the families chore_fit_*, chore_so3_*, chore_contact_*,
chore_smpl_lbs_*, chore_landmarks_* and chore_eval_*: the ids of the cases that call it, or the reason none does.
tests/test_fit_coverage_table.py holds the table against _lib.py, the constants against the .hip sources and the case
families against the GPU test module."""
import zlib

import numpy as np

# ---- the constants the shapes were chosen around (held equal to the sources by test_fit_coverage_table.py) ----
CONSTANTS = {
    "FB": 4,                 # smpl_lbs.hip: frames a vertex / reduction workgroup handles together
    "VF_V": 64,              # smpl_lbs.hip: vertices per workgroup of the forward vertex kernel
    "LBS_BWD_BLOCK": 256,    # smpl_lbs.hip: vertices per workgroup of the backward vertex kernel
    "TILE": 256,             # contact.hip: queries and candidates per workgroup
    "CP_MAX": 32,            # contact.hip: most parts
    "PT_BLOCK": 256,         # fit_terms.hip: points per workgroup of the point / object kernels
    "PT_MAXC": 16,           # fit_terms.hip: most classes of the cross entropy
    "FS_MAXT": 16,           # fit_step.hip: most tensors of one Adam launch
    "FS_MAXL": 16,           # fit_step.hip: most terms of one weighted sum
    "ADAM_BLOCK": 256,       # fit_step.hip: threads per workgroup of the Adam launch ...
    "ADAM_MAX_BLOCKS": 64,   # ... and the cap of its grid: more than 64 * 256 = 16 384 elements run the grid-stride loop
    "NN_TILE": 1024,         # eval_metrics.hip: candidates per LDS tile
    "NN_BLOCK": 256,         # eval_metrics.hip: queries per workgroup
    "SO3_PER_BLOCK": 64,     # so3.hip: matrices per workgroup
}
V_SMPL, J_SMPL, NB_SMPL = 6890, 52, 10
THRES = 0.08                 # contact threshold of the fit


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


CASES = {}


def _add(family, name, **kw):
    CASES.setdefault(family, []).append(dict(kw, id="%s.%s" % (family, name), family=family))


def ids(family):
    return [c["id"] for c in CASES[family]]


# ================================================================================================ chore_smpl_lbs_fwd / _bwd
# B = 1, 3: one short group; 4: one full group; 5, 9: full groups and a last one of a single frame (the row clamp of lbs_dpm_body,
# the early exit of lbs_reduce_kernel)
for _B in (1, 3, 4, 5, 9):
    for _offs in (0, 1):
        for _up in ("verts", "joints", "both"):
            _add("lbs", "B%d.%s.%s" % (_B, "offsets" if _offs else "plain", _up), B=_B, offsets=_offs, up=_up, pose="random",
                 scale=0.9 if _offs else 1.0)
for _pose in ("zero", "tiny", "near_pi", "zero_betas"):
    _add("lbs", "pose_%s" % _pose, B=5, offsets=int(_pose in ("tiny", "zero_betas")), up="both", pose=_pose, scale=1.0)


def lbs_inputs(c):
    """-> pose (B,156), betas (B,10), trans (B,3), offsets (B,V,3) or None, g_verts or None, g_joints or None"""
    from chore_amd.utils import synth
    B = c["B"]
    pose, betas, trans = synth.synth_smpl_params(B, seed=17 + B)
    r = rng("lbs", c["id"])
    if c["pose"] == "zero":
        pose = np.zeros_like(pose)
    elif c["pose"] == "tiny":
        pose = np.full_like(pose, 1e-6)
    elif c["pose"] == "near_pi":          # one joint of every frame turned by pi - 1e-3 about a random axis
        for b in range(B):
            ax = r.standard_normal(3)
            pose[b, 3 * (b * 7 % J_SMPL):3 * (b * 7 % J_SMPL) + 3] = ax / np.linalg.norm(ax) * (np.pi - 1e-3)
    elif c["pose"] == "zero_betas":
        betas = np.zeros_like(betas)
    offs = _f32(r.standard_normal((B, V_SMPL, 3)) * 0.003) if c["offsets"] else None
    gv = _f32(r.standard_normal((B, V_SMPL, 3))) if c["up"] in ("verts", "both") else None
    gj = _f32(r.standard_normal((B, J_SMPL, 3))) if c["up"] in ("joints", "both") else None
    return _f32(pose), _f32(betas), _f32(trans), offs, gv, gj


# ================================================================================================ chore_fit_smpl_terms_fwd / _bwd
# one workgroup loops over the frames; R = 25 (the keypoint rows alone), 137 (the fit's), 256 (one row per thread, the most)
for _B in (1, 3, 8):
    for _R in (25, 137, 256):
        _add("smpl_terms", "B%d.R%d" % (_B, _R), B=_B, R=_R, kpts=True, null_up=None, conf_zero=False)
_add("smpl_terms", "no_kpts", B=3, R=137, kpts=False, null_up=None, conf_zero=False)
for _k, _n in enumerate(("pose", "hand", "pinit", "smplz", "j2d")):
    _add("smpl_terms", "null_up_%s" % _n, B=3, R=137, kpts=True, null_up=_k, conf_zero=False)
_add("smpl_terms", "conf_zero", B=3, R=25, kpts=True, null_up=None, conf_zero=True)
SMPL_TERMS_REFUSED = [dict(B=2, P=156, R=24), dict(B=2, P=156, R=257), dict(B=2, P=72, R=137), dict(B=2, P=157, R=137)]
CAM8 = tuple(float(np.float32(v)) for v in (979.7844, 979.840, 1018.952, 779.486, 600.0, 1200.0, 512.0, 2.2))


def smpl_terms_inputs(c):
    """-> dict of float32 arrays: pose, pose_init, J, kpts (or None), cc, bmean, bprec, hmean, lprec, rprec, up (5)"""
    r = rng("smpl_terms", c["id"])
    B, R = c["B"], c["R"]
    d = {}
    d["pose"] = _f32(r.standard_normal((B, 156)) * 0.25)
    d["pose_init"] = _f32(d["pose"][:, 3:72] + r.standard_normal((B, 69)) * 0.1)
    J = r.standard_normal((B, R, 3)) * np.array([0.4, 0.6, 0.15]) + np.array([0.0, 0.3, 2.3])
    d["J"] = _f32(J)
    d["cc"] = _f32(np.array([1008.0, 995.0]) + r.standard_normal((B, 2)) * 20)
    fx, fy, cx, cy, hc, crop, net, _ = CAM8
    proj = np.stack([hc + fx * J[:, :25, 0] / J[:, :25, 2] + cx - d["cc"][:, 0:1], hc + fy * J[:, :25, 1] / J[:, :25, 2] + cy - d["cc"][:, 1:2]],
                    -1) * net / crop
    conf = np.zeros((B, 25, 1)) if c["conf_zero"] else r.uniform(0.0, 1.0, (B, 25, 1)) * (r.uniform(0, 1, (B, 25, 1)) > 0.2)
    d["kpts"] = _f32(np.concatenate([proj + r.standard_normal((B, 25, 2)) * 20.0, conf], -1)) if c["kpts"] else None
    d["bmean"] = _f32(r.standard_normal(63) * 0.1)
    d["bprec"] = _f32(np.tril(r.standard_normal((63, 63)) * 0.3) + np.eye(63))
    d["hmean"] = _f32(r.standard_normal(90) * 0.1)
    d["lprec"] = _f32(np.eye(45) + r.standard_normal((45, 45)) * 0.05)
    d["rprec"] = _f32(np.eye(45) + r.standard_normal((45, 45)) * 0.05)
    d["up"] = [None if c["null_up"] == k else np.float32(v) for k, v in enumerate(r.uniform(0.5, 2.0, 5))]
    return d


# ================================================================================================ chore_fit_point_terms_fwd / _bwd
# N = 1; 255, 256, 257: around the 256-thread block; 1000: four blocks, the last ragged.  C = 1, the fit's 14, PT_MAXC = 16.
CLAMPS = {0: 0.1, 1: 0.8}
_i = 0
for _N in (1, 255, 256, 257, 1000):
    for _B in (1, 3):
        for _C in (1, 14, 16):
            _add("point_terms", "N%d.B%d.C%d" % (_N, _B, _C), N=_N, B=_B, C=_C, channel=_i % 2, logits="normal", null_up=None)
            _i += 1
for _N, _B in ((1, 3), (255, 1), (256, 3), (257, 1), (1000, 3)):
    _add("point_terms", "N%d.B%d.no_logits" % (_N, _B), N=_N, B=_B, C=0, channel=_N % 2, logits=None, null_up=None)
_add("point_terms", "logits_pm80", N=257, B=3, C=14, channel=0, logits="pm80", null_up=None)
_add("point_terms", "null_up_clamped", N=257, B=3, C=14, channel=1, logits="normal", null_up=0)
_add("point_terms", "null_up_ce", N=257, B=3, C=14, channel=0, logits="normal", null_up=1)
_add("point_terms", "null_up_clamped_no_logits", N=255, B=1, C=0, channel=0, logits=None, null_up=0)


def point_terms_inputs(c):
    """-> df (B,2,N), cmax, logits (B,C,N) or None, labels (B,N) int64 or None, up (2); a tenth of the distances sit exactly on
    the clamp, where the gradient passes (as torch.clamp's does)"""
    r = rng("point_terms", c["id"])
    B, N, C, ch = c["B"], c["N"], c["C"], c["channel"]
    cmax = np.float32(CLAMPS[ch])
    df = _f32(r.uniform(0.0, 2.0 * CLAMPS[ch], (B, 2, N)))
    df[:, ch][r.uniform(0, 1, (B, N)) < 0.1] = cmax
    if N == 1:
        df[0, ch, 0] = cmax
    logits = labels = None
    if c["logits"]:
        logits = _f32(r.standard_normal((B, C, N)) * 2.0)
        if c["logits"] == "pm80":
            logits = _f32(np.where(r.uniform(0, 1, (B, C, N)) < 0.5, -80.0, 80.0) + logits)
        labels = r.integers(0, C, (B, N)).astype(np.int64)
    up = [None if c["null_up"] == k else np.float32(v) for k, v in enumerate(r.uniform(0.5, 2.0, 2))]
    return df, cmax, logits, labels, up


# ================================================================================================ chore_fit_obj_transform / _obj_terms
# N = 1; 255, 257: around the block; 3000: the fit's, twelve strides of the one-workgroup-per-frame reductions
for _N in (1, 255, 257, 3000):
    for _B in (1, 3):
        _add("obj_transform", "N%d.B%d" % (_N, _B), N=_N, B=_B)
        _add("obj_terms", "N%d.B%d" % (_N, _B), N=_N, B=_B, null_up=None)
_add("obj_terms", "null_up_scale", N=257, B=3, null_up=0)
_add("obj_terms", "null_up_ocent", N=257, B=3, null_up=1)
SCALE0 = float(np.float32(0.93))


def _rotations(r, B):
    q, _ = np.linalg.qr(r.standard_normal((B, 3, 3)))
    return q * np.sign(np.linalg.det(q))[:, None, None]


def obj_transform_inputs(c):
    """-> verts (B,N,3), R (B,3,3), t (B,3), s (B), g (B,N,3)"""
    r = rng("obj_transform", c["id"])
    B, N = c["B"], c["N"]
    return (_f32(r.standard_normal((B, N, 3)) * 0.3), _f32(_rotations(r, B) + r.standard_normal((B, 3, 3)) * 0.01),
            _f32(r.standard_normal((B, 3)) * 0.2 + np.array([0.1, 0.3, 2.2])), _f32(r.uniform(0.8, 1.2, B)), _f32(r.standard_normal((B, N, 3))))


def obj_terms_inputs(c):
    """-> object (B,N,3), centers (B,6,N), obj_s (B), smpl_center (B,3), up (2)"""
    r = rng("obj_terms", c["id"])
    B, N = c["B"], c["N"]
    obj = _f32(r.standard_normal((B, N, 3)) * 0.3 + np.array([0.3, 0.2, 2.4]))
    centers = _f32(r.standard_normal((B, 6, N)) * 0.2 + np.array([0.0, 0.0, 0.0, 0.1, -0.2, 0.3])[None, :, None])
    up = [None if c["null_up"] == k else np.float32(v) for k, v in enumerate(r.uniform(0.5, 2.0, 2))]
    return obj, centers, _f32(r.uniform(0.8, 1.2, B)), _f32(r.standard_normal((B, 3)) * 0.1 + np.array([0.0, 0.3, 2.2])), up


# ================================================================================================ chore_so3_project_fwd / _bwd
SO3_CONTENT = ("rotation", "twice_rotation", "minus_identity", "diag_1_1_m1", "diag_2_1_1em6", "rank2_exact", "rank2_near", "random")
for _content in SO3_CONTENT:
    _add("so3", "B1.%s" % _content, B=1, content=(_content,))
for _B in (64, 65, 130):          # one full workgroup; one matrix in a second; two full workgroups and two matrices
    _add("so3", "B%d.mixed" % _B, B=_B, content=SO3_CONTENT)


def so3_inputs(c):
    """-> M (B,3,3), G (B,3,3) float32: the named matrices first, seeded random ones after them.  No matrix of rank <= 1: those are
    outside the contract of so3.hip (the result is then not a rotation)"""
    r = rng("so3", c["id"])
    B = c["B"]
    M = r.standard_normal((B, 3, 3))
    rot = _rotations(r, 2)
    named = {"rotation": rot[0], "twice_rotation": 2.0 * rot[1], "minus_identity": -np.eye(3), "diag_1_1_m1": np.diag([1.0, 1.0, -1.0]),
             "diag_2_1_1em6": np.diag([2.0, 1.0, 1e-6]), "rank2_exact": np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 4.0], [1.0, 0.0, -2.0]]),
             "rank2_near": np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]) + np.outer([-2.0, 0.3, 1.0], [1.0, 1.0, -0.7])}
    for i, name in enumerate(c["content"]):
        if name != "random":
            M[i] = named[name]
    return _f32(M), _f32(r.standard_normal((B, 3, 3)))


# ================================================================================================ chore_contact_fwd / _bwd
# (1, 1): a single point each; (255, 257): a tile minus / plus one; (256, 256): exactly one tile each; (513, 40): three query tiles
# against less than one; (700, 300): the existing case's.  P = 1, the fit's 14, CP_MAX = 32.  B = 3 runs the three kinds of frame:
# ordinary, no contact at all (skipped), no contact on the human side (every vertex takes part)
for _Nh, _No in ((1, 1), (255, 257), (256, 256), (513, 40), (700, 300)):
    for _P in (1, 14, 32):
        for _B in (1, 3):
            _add("contact", "h%d.o%d.P%d.B%d" % (_Nh, _No, _P, _B), Nh=_Nh, No=_No, P=_P, B=_B, frames="mixed" if _B == 3 else "plain",
                 null=None)
_add("contact", "d_hum_null", Nh=700, No=300, P=14, B=3, frames="mixed", null="hum")
_add("contact", "d_obj_null", Nh=700, No=300, P=14, B=3, frames="mixed", null="obj")
_add("contact", "no_contact_frame", Nh=255, No=257, P=14, B=1, frames="none", null=None)
_add("contact", "object_side_empty", Nh=255, No=257, P=14, B=1, frames="obj_none", null=None)
_add("contact", "part_on_one_side", Nh=255, No=257, P=14, B=1, frames="one_sided_part", null=None)
_add("contact", "single_pair_part", Nh=255, No=257, P=14, B=1, frames="single_pair", null=None)
CONTACT_REFUSED_P = 33
CONTACT_TIE_CAP = 0.005          # at most this share of the participating points may sit on a nearest-neighbour tie


def contact_inputs(c):
    """-> hum (B,Nh,3), obj (B,No,3), df_h (B,Nh), df_o (B,No), labels (Nh) int32, logits (B,P,No), g (upstream gradient).
    No distance lies within 1e-3 of the threshold and (continuous draws) no two logits of a point tie."""
    r = rng("contact", c["id"])
    B, Nh, No, P = c["B"], c["Nh"], c["No"], c["P"]
    hum, obj = r.standard_normal((B, Nh, 3)) * 0.3, r.standard_normal((B, No, 3)) * 0.3 + 0.1
    df_h, df_o = r.uniform(0, 0.3, (B, Nh)), r.uniform(0, 0.3, (B, No))
    for df in (df_h, df_o):
        df[np.abs(df - THRES) < 1e-3] = 0.05
    if Nh == 1:
        df_h[:], df_o[:] = 0.01, 0.02
    logits = r.standard_normal((B, P, No))
    labels = r.integers(0, P, Nh)
    fr = c["frames"]
    if fr == "mixed":
        df_h[1], df_o[1] = 1.0, 1.0
        df_h[2] = 1.0
    elif fr == "none":
        df_h[:], df_o[:] = 1.0, 1.0
    elif fr == "obj_none":
        df_o[:] = 1.0
    elif fr == "one_sided_part":
        logits[:, P - 1] = -50.0                     # never predicted on the object
        labels[:8] = P - 1                           # present, and in contact, on the body
        df_h[:, :8] = 0.01
    elif fr == "single_pair":                        # part 0: exactly one participating point on each side
        labels[labels == 0] = 1
        labels[3] = 0
        df_h[:, 3] = 0.01
        logits[:, 0] = -50.0
        logits[:, 0, 5] = 50.0
        df_o[:, 5] = 0.01
    return _f32(hum), _f32(obj), _f32(df_h), _f32(df_o), labels.astype(np.int32), _f32(logits), np.float32(r.uniform(0.5, 3.0))


# ================================================================================================ chore_fit_adam_step / _acc
# n = 1; 255, 257: around a workgroup; 16 385: one more than 64 workgroups hold; 40 000: three passes of the grid-stride loop, the last
# ragged.  nt = 1 and FS_MAXT = 16 (the other tensors of a 16-tensor launch take the sizes of ADAM_OTHERS in turn).
ADAM_OTHERS = (3, 72, 256, 1000, 10, 17000, 9)
_i = 0
for _n in (1, 255, 257, 16385, 40000):
    for _nt in (1, 16):
        _add("adam", "n%d.nt%d" % (_n, _nt), n=_n, nt=_nt, api="acc" if _i % 2 else "step", frozen=False, counted=int(_i % 4 == 1),
             slices=False, acc_only=False)
        _i += 1
_add("adam", "frozen.step", n=257, nt=16, api="step", frozen=True, counted=0, slices=False, acc_only=False)
_add("adam", "frozen.acc", n=16385, nt=1, api="acc", frozen=True, counted=1, slices=False, acc_only=False)
_add("adam", "acc_only_leaves", n=257, nt=16, api="acc", frozen=False, counted=0, slices=False, acc_only=True)
_add("adam", "column_slices", n=40000, nt=16, api="acc", frozen=False, counted=1, slices=True, acc_only=False)
_add("adam", "column_slices_small", n=255, nt=1, api="acc", frozen=False, counted=0, slices=True, acc_only=False)
ADAM_HYPER = dict(lr=0.02, b1=0.9, b2=0.999, eps=1e-8)
ADAM_STEPS = 3


def adam_layout(c):
    """-> per tensor (n, cols, pstride, accumulate-only): tensor 0 has the case's size; a column slice has rows of `cols` elements
    `pstride` apart in a wider storage"""
    out = []
    for k in range(c["nt"]):
        n = c["n"] if k == 0 else ADAM_OTHERS[(k - 1) % len(ADAM_OTHERS)]
        cols = pstride = n
        if c["slices"] and k % 2 == 0:
            cols = next(d for d in (63, 50, 45, 17, 5, 3, 1) if n % d == 0)
            pstride = cols + 9
        out.append((n, cols, pstride, bool(c["acc_only"] and k % 3 == 1)))
    return out


# ================================================================================================ stop rule, weighted sum (one thread each)
_add("step", "rule_table", kind="rule")
for _n in (1, 16):
    _add("step", "weighted_sum.n%d" % _n, kind="sum", n=_n)
    _add("step", "fused.n%d" % _n, kind="fused", n=_n)
# (armed, already stopped, hit): every combination; a hit is a loss within prev^2 * tol of prev
RULE_TABLE = [(a, s, h) for a in (0, 1) for s in (0, 1) for h in (0, 1)]
RULE_TOL = 1e-3


def rule_values(hit, r):
    prev = np.float32(r.uniform(2.0, 30.0))
    rel = 0.2 * prev * RULE_TOL if hit else 5.0 * prev * RULE_TOL
    return np.float32(prev * (1.0 + rel * (1 if r.uniform() < 0.5 else -1))), prev


# ================================================================================================ chore_eval_*
# chamfer: (1, 1); (255, 1025): a query block minus one against a candidate tile plus one; (1024, 1024): exact tiles; (2049, 300): nine
# query blocks, the last of one point, against a third of a tile
for _Nx, _Ny in ((1, 1), (255, 1025), (1024, 1024), (2049, 300)):
    _add("chamfer", "x%d.y%d" % (_Nx, _Ny), Nx=_Nx, Ny=_Ny, dup=False)
_add("chamfer", "duplicates", Nx=300, Ny=257, dup=True)
for _N in (3, 255, 257, 1500):
    _add("procrustes", "N%d" % _N, N=_N, kind="generic")
_add("procrustes", "planar", N=257, kind="planar")
_add("procrustes", "reflected", N=257, kind="reflected")
_add("procrustes", "offset_1e3", N=257, kind="offset")


def chamfer_inputs(c):
    r = rng("chamfer", c["id"])
    x, y = r.standard_normal((c["Nx"], 3)), r.standard_normal((c["Ny"], 3)) * 0.8 + 0.2
    if c["dup"]:                      # points that occur twice in a cloud, and points shared by the two clouds
        x[100:150] = x[:50]
        y[:40] = x[200:240]
        y[250:] = y[41:48]
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def procrustes_inputs(c):
    """-> S1, S2 (N,3) float64: S2 a similarity image of S1 plus noise"""
    r = rng("procrustes", c["id"])
    N = c["N"]
    S1 = r.standard_normal((N, 3)) * np.array([0.3, 0.8, 0.2])
    if c["kind"] == "planar":
        S1[:, 2] = 0.0
        S1 = S1 @ _rotations(r, 1)[0].T       # a plane in general position: K = X1 X2^T has rank 2
    Q = _rotations(r, 1)[0]
    if c["kind"] == "reflected":
        Q = Q @ np.diag([1.0, 1.0, -1.0])     # the best orthogonal map is a reflection; the rotation asked for is not
    S2 = 1.7 * S1 @ Q.T + np.array([0.2, -0.1, 2.0]) + r.standard_normal((N, 3)) * 0.01
    if c["kind"] == "offset":
        S1 = S1 + 1e3
        S2 = S2 - 1e3
    return np.ascontiguousarray(S1), np.ascontiguousarray(S2)


# ================================================================================================ the coverage table
_ELSEWHERE_LANDMARKS = ("out of scope here: tests/test_gpu_smpl.py::test_landmark_regression_forward_and_backward compares it with a float64 "
                        "product at B = 1, 3 with dense and sparse rows, and the fit's landmark call at B = 2 runs in test_gpu_fit.py")
COVERAGE = {
    "chore_smpl_lbs_fwd": ids("lbs"),
    "chore_smpl_lbs_bwd": ids("lbs"),
    "chore_landmarks_fwd": _ELSEWHERE_LANDMARKS,
    "chore_landmarks_bwd": _ELSEWHERE_LANDMARKS,
    "chore_fit_smpl_terms_fwd": ids("smpl_terms"),
    "chore_fit_smpl_terms_bwd": ids("smpl_terms"),
    "chore_fit_point_terms_workspace_bytes": ids("point_terms"),
    "chore_fit_point_terms_fwd": ids("point_terms"),
    "chore_fit_point_terms_bwd": ids("point_terms"),
    "chore_fit_obj_transform_fwd": ids("obj_transform"),
    "chore_fit_obj_transform_bwd": ids("obj_transform"),
    "chore_fit_obj_terms_workspace_bytes": ids("obj_terms"),
    "chore_fit_obj_terms_fwd": ids("obj_terms"),
    "chore_fit_obj_terms_bwd": ids("obj_terms"),
    "chore_fit_rot_noise": ("one launch of one workgroup whose only shape is B * 9 elements: test_gpu_fit.py::test_rot_noise_operator holds it "
                            "bit-equal to the tensor expression, counter and gradient included"),
    "chore_so3_aux_bytes": ids("so3"),
    "chore_so3_project_fwd": ids("so3"),
    "chore_so3_project_bwd": ids("so3"),
    "chore_contact_workspace_bytes": ids("contact"),
    "chore_contact_fwd": ids("contact"),
    "chore_contact_bwd": ids("contact"),
    "chore_fit_adam_step": [c["id"] for c in CASES["adam"] if c["api"] == "step"],
    "chore_fit_adam_step_acc": [c["id"] for c in CASES["adam"] if c["api"] == "acc"],
    "chore_fit_stop_rule": [c["id"] for c in CASES["step"] if c["kind"] in ("rule", "fused")],
    "chore_fit_weighted_sum": [c["id"] for c in CASES["step"] if c["kind"] in ("sum", "fused")],
    "chore_fit_weighted_sum_bwd": [c["id"] for c in CASES["step"] if c["kind"] in ("sum", "fused")],
    "chore_fit_weighted_sum_step": [c["id"] for c in CASES["step"] if c["kind"] == "fused"],
    "chore_eval_chamfer_workspace_bytes": ids("chamfer"),
    "chore_eval_chamfer": ids("chamfer"),
    "chore_eval_procrustes": ids("procrustes"),
    "chore_eval_apply_similarity": ids("procrustes"),
}
FAMILIES = ("chore_fit_", "chore_so3_", "chore_contact_", "chore_smpl_lbs_", "chore_landmarks_", "chore_eval_")
