"""GPU: every query kernel behind chore_query_fwd[_ws], chore_query_fwd_train, chore_query_bwd_points, chore_gen_surface_step_fused and
chore_query_bwd_train (the 56 instantiations of csrc/query_fwd.hip and csrc/query_bwd.hip) against the float64 reference of
tests/query_ref.py, at every launch plan csrc/query_plan.h can decide on.

Cases: tests/query_kernel_cases.py (one per distinct plan and switch set, the ragged counts, the tile rules' edges).  The library reads
its switches once per process, so every switch set runs in a child of its own (this file with --child, tests/gpu_child.py): the
parent makes all inputs on the CPU and hands them over in an .npz, so device and reference see the same bits; a reference forward is
computed once per (points, maps).  A child runs once, under a time limit of its own; after an abnormal end no later child starts.

The child, per call
  * asks chore_query_plan (switches from ITS environment) and asserts the plan of the kernel name the case is filed under: a value
    check below is known to have run that instantiation;
  * hands over output buffers filled with NaN inside sentinel margins (the staging: NaN bytes inside sentinel pages).

Checks per case (bounds and exclusions: query_kernel_cases.py; every exclusion is a condition on the reference alone; excluded
points must still be finite)
  forward            df, pca, parts, centers; in_img and the df == 5.0 mask identical to the reference's outside the border exclusion
  training forward   also X -- bit for bit what query_ref.features_f32 gives, the float32 restatement operation by operation -- and H,
                     values and zero pattern
  sort               the workspace holds a permutation of 0..N-1 per image; same bounds; bit-identical to the call without workspace
  backward           dpoints; exact zeros outside the image where df's is the only gradient; absent heads are absent in the reference
  surface step       the displacement out - p for k = 0 and k = 1; outside the image exactly min(5, thr) times a zero gradient: no move
  training backward  dZ, dX, dpoints, and the X and H its staging holds (written by the forward, or by the recompute kernel itself)

Measured on an MI355X: the largest error over the cases of a switch set, next to its bound, in units of max(1, max |ref|) for the
outputs, X and H and of max |ref| for the gradients (65 / 65 / 62 / 62 calls under none / W4 / NOSPLIT / NO_ONE_HEAD; the four
tests take 39 s, 9 s of it the children)
  operation          quantity       none, W4             NOSPLIT              NO_ONE_HEAD
  forward            four outputs   2.46e-05 (5e-5)      5.08e-06 (5e-5)      2.46e-05 (5e-5)      the sort cases, 128 x 128 maps
  training forward   four outputs   4.04e-06 (5e-5)      4.04e-06             4.04e-06
                     X, H           5.47e-06, 5.05e-06 (5e-5) in every set; X bit for bit the float32 restatement
  backward           dpoints        4.70e-06 (2e-5)      4.70e-06             4.70e-06
  surface step       displacement   1.75e-05 (2e-5)      1.75e-05             8.38e-06 (2e-5)      where the bound is the issue's
                                    3.76e-05 (1.4e-4)    3.76e-05             8.19e-05 (2.9e-4)    where FLOORS sets it (4 x 4097, 4 x 6200)
  training backward  dZ, dX         3.16e-07, 4.36e-07 (2e-5) in every set
                     dpoints        6.14e-06 (2e-5) in every set
The forward's error on 128 x 128 maps and the step's are float32's own (query_ref in float32: 2.4e-05 and 1.6e-05 .. 7.6e-05 at the
same cases): the rounding of the sample coordinates, which a kernel that follows the reference operation by operation shares.
Mutation check (scratch builds, not kept): launch_query_bwd handing the kernel one_head + 1, store_tile skipping the second column
block of the NCB = 2 kernels, and the staged backward reading layer 1's ReLU bits for layer 2 each fail test_switch_set[none]
(dpoints of all seven one-head backward cases wrong at every point; H and dZ of the training backward not written; dZ, dX and
dpoints of the four staged training backward cases wrong).
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_child                 # noqa: E402
import query_kernel_cases as kc  # noqa: E402
import query_plan_cases as qc    # noqa: E402
import query_ref as qr           # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL, MARGIN = 7.0, 256                  # floats before and after every output
PAGE, PAGE_BYTE = 4096, 0xA5                 # bytes before and after the staging and the workspace
CHILD_TIMEOUT = 240
API_ORDER = (0, 2, 1, 3)                     # the entry points take df, pca, parts, centers; heads are df, parts, pca, centers
OUT_DIM = qr.OUT_DIM
XH_FLOATS = qr.KPAD + 3 * 4 * qr.HID         # floats per point of X and H (and of dX and dZ) in the staging

RUNNER = gpu_child.ChildRunner(__file__, lambda name: name.startswith("CHORE_QUERY"))


def _keys(c):
    mt = kc.map_type(c[1])
    return "maps/%d/%dx%d" % (mt, c[4], c[5]), "pts/%dx%d" % (c[2], c[3])


# ------------------------------------------------------------------------------------------------ the reference, cached
_FWD = {}


def ref_forward(c):
    """query_ref.forward of a case's points and maps; the last few are kept (the jobs of a set are ordered by this key)"""
    key = (kc.map_type(c[1]), c[4], c[5], c[2], c[3])
    if key not in _FWD:
        while len(_FWD) >= 3:
            _FWD.pop(next(iter(_FWD)))
        feat, tmpx = kc.maps_of(*key[:3])
        pts, cc = kc.points_of(c[2], c[3])
        _FWD[key] = qr.forward(pts, cc, feat[:c[2]], tmpx[:c[2]], kc.weights())
    return _FWD[key]


def thresholds(c):
    f = ref_forward(c)
    return [kc.surface_thr(f, k) for k in (0, 1)]


# ------------------------------------------------------------------------------------------------ the child process
def child_main(in_path, job_path, out_path):
    from chore_amd import _lib
    jobs = json.load(open(job_path))
    data = np.load(in_path)
    dev = torch.device("cuda", 0)
    h, L = _lib.handle(0), _lib.lib
    stream = torch.cuda.current_stream().cuda_stream
    tdt = {qc.F32: torch.float32, qc.BF16: torch.bfloat16, qc.F16: torch.float16}
    out, cache = {}, {}

    def dev_of(key, dt=torch.float32):
        if (key, dt) not in cache:
            cache[key, dt] = torch.from_numpy(data[key]).to(dev).to(dt).contiguous()
        return cache[key, dt]

    named = [(k[2:], dev_of(k)) for k in data.files if k.startswith("w/")]
    arena = torch.empty(L.chore_heads_arena_bytes(_lib.F32), dtype=torch.uint8, device=dev)
    descs, keep = _lib.make_descs(named)
    _lib.check(L.chore_heads_pack(h, descs, len(named), _lib.F32, arena.data_ptr(), stream), h, "chore_heads_pack")
    cam6 = (ctypes.c_float * 6)(*qr.CAM6)

    def guarded(*shape, dt=torch.float32):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * MARGIN,), SENTINEL if dt == torch.float32 else PAGE_BYTE, dtype=dt, device=dev)
        buf[MARGIN:MARGIN + n] = float("nan") if dt == torch.float32 else 0xEE
        return buf, buf.data_ptr() + MARGIN * buf.element_size()

    def paged(nbytes):
        buf = torch.full((nbytes + 2 * PAGE,), PAGE_BYTE, dtype=torch.uint8, device=dev)
        buf[PAGE:PAGE + nbytes] = 0xFF             # NaN as floats
        return buf, buf.data_ptr() + PAGE

    def plan(op, dtype, B, N, FH, FW, live, flags, name, sort):
        got = (ctypes.c_int * 9)()
        n = L.chore_query_plan(op, dtype, B, N, FH, FW, live, flags, -1, got, 9)
        want = qc.plan_of_name(name, sort, live)
        assert n == 9 and list(got) == want, ("the plan is not the one the case is filed under", name, sort, list(got[:max(n, 0)]), want)

    for cid, op, dtype, B, N, FH, FW, live, flags, name, sort, thr in jobs:
        mkey, pkey = _keys((op, dtype, B, N, FH, FW))
        mt = kc.map_type(dtype)
        feat, tmpx = dev_of(mkey + "/feat", tdt[mt])[:B].contiguous(), dev_of(mkey + "/tmpx", tdt[mt])[:B].contiguous()
        pts, cc = dev_of(pkey), dev_of("cc")[:B].contiguous()
        head = (h, pts.data_ptr(), cc.data_ptr(), B, N, feat.data_ptr(), FH, FW, tmpx.data_ptr(), kc.TH, kc.TW, dtype, arena.data_ptr(), cam6)
        g = [dev_of("g/%s/%d" % (cid, i)) if live >> i & 1 else None for i in range(4)]
        gp = [None if g[i] is None else g[i].data_ptr() for i in API_ORDER]

        def outputs():
            bufs = [guarded(B, OUT_DIM[i], N) for i in API_ORDER] + [guarded(B, N, dt=torch.uint8)]
            return [b for b, _ in bufs], [p for _, p in bufs]

        def keep_outputs(tag, bufs):
            for nm, b in zip(("df", "pca", "parts", "centers", "in_img"), bufs):
                out["%s|%s%s" % (cid, tag, nm)] = b.cpu().numpy()

        def keep_staging(buf, parts):
            P, f = B * N, buf[PAGE:PAGE + 4 * (2 * B * N * XH_FLOATS)].view(torch.float32)
            o = {"X": (0, P * qr.KPAD), "H": (P * qr.KPAD, P * XH_FLOATS), "dZ": (P * XH_FLOATS, P * XH_FLOATS + P * 12 * qr.HID),
                 "dX": (P * XH_FLOATS + P * 12 * qr.HID, 2 * P * XH_FLOATS)}
            for nm in parts:
                out["%s|%s" % (cid, nm)] = f[o[nm][0]:o[nm][1]].cpu().numpy()
            out[cid + "|pages"] = torch.cat([buf[:PAGE], buf[-PAGE:]]).cpu().numpy()

        def fwd_train(staging_ptr, ptrs):
            return L.chore_query_fwd_train(*head, *ptrs, staging_ptr, stream)

        if op == qc.FWD:
            plan(op, dtype, B, N, FH, FW, live, flags, name, sort)
            bufs, ptrs = outputs()
            ws = ws_ptr = None
            if flags & qc.WS:
                nws = L.chore_query_fwd_workspace_bytes(B, N)
                ws, ws_ptr = paged(nws)
            _lib.check(L.chore_query_fwd_ws(*head, *ptrs, ws_ptr, stream), h, cid)
            torch.cuda.synchronize()
            keep_outputs("", bufs)
            if ws is not None:
                out[cid + "|perm"] = ws[PAGE:PAGE + 4 * B * N].view(torch.int32).cpu().numpy()
                out[cid + "|pages"] = torch.cat([ws[:PAGE], ws[-PAGE:]]).cpu().numpy()
                plan(op, dtype, B, N, FH, FW, live, flags & ~qc.WS, name, 0)       # the same call without a workspace
                bufs, ptrs = outputs()
                _lib.check(L.chore_query_fwd_ws(*head, *ptrs, None, stream), h, cid + " without workspace")
                torch.cuda.synchronize()
                keep_outputs("plain/", bufs)
        elif op == qc.FWD_TRAIN:
            plan(op, dtype, B, N, FH, FW, live, flags, name, sort)
            bufs, ptrs = outputs()
            st, st_ptr = paged(L.chore_query_train_bytes(B, N))
            _lib.check(fwd_train(st_ptr, ptrs), h, cid)
            torch.cuda.synchronize()
            keep_outputs("", bufs)
            keep_staging(st, ("X", "H"))
        elif op == qc.BWD_POINTS:
            plan(op, dtype, B, N, FH, FW, live, flags, name, sort)
            dp, dp_ptr = guarded(B, N, 3)
            _lib.check(L.chore_query_bwd_points(*head, *gp, dp_ptr, stream), h, cid)
            torch.cuda.synchronize()
            out[cid + "|dpoints"] = dp.cpu().numpy()
        elif op == qc.SURFACE_STEP:
            plan(op, dtype, B, N, FH, FW, live, flags, name, sort)
            for k in (0, 1):
                o, o_ptr = guarded(B, N, 3)
                _lib.check(L.chore_gen_surface_step_fused(*head, k, thr[k], o_ptr, stream), h, cid)
                torch.cuda.synchronize()
                out["%s|step%d" % (cid, k)] = o.cpu().numpy()
        else:
            st, st_ptr = paged(L.chore_query_train_bytes(B, N))
            if flags & qc.HF:           # the staged backward reads the training forward of the same inputs (a case of its own in this set)
                _, ptrs = outputs()
                _lib.check(fwd_train(st_ptr, ptrs), h, cid + " forward")
            plan(op, dtype, B, N, FH, FW, live, flags, name, sort)
            dp, dp_ptr = guarded(B, N, 3)
            _lib.check(L.chore_query_bwd_train(*head, *gp, st_ptr, dp_ptr, 1 if flags & qc.HF else 0, stream), h, cid)
            torch.cuda.synchronize()
            out[cid + "|dpoints"] = dp.cpu().numpy()
            keep_staging(st, ("X", "H", "dZ", "dX"))
    np.savez(out_path, **out)


def run_child(tmp_path, k):
    name, _, env = qc.SWITCH_SETS[k]
    arrays, jobs = {}, []
    for c, kname, sort in kc.jobs_of(k):
        mkey, pkey = _keys(c)
        if mkey + "/feat" not in arrays:
            arrays[mkey + "/feat"], arrays[mkey + "/tmpx"] = kc.maps_of(kc.map_type(c[1]), c[4], c[5])
        if pkey not in arrays:
            arrays[pkey] = kc.points_of(c[2], c[3])[0]
        cid = kc.case_id(c)
        for i, g in enumerate(kc.grads_of(c)):
            if g is not None:
                arrays["g/%s/%d" % (cid, i)] = g
        jobs.append((cid,) + tuple(c[:8]) + (kname, sort, thresholds(c) if c[0] == qc.SURFACE_STEP else None))
    arrays["cc"] = np.tile(np.array([kc.CROP_CENTER], np.float32), (4, 1))
    for n, w in kc.weights().items():
        arrays["w/" + n] = w
    return RUNNER.run(tmp_path, name, env, arrays, jobs, CHILD_TIMEOUT)


# ------------------------------------------------------------------------------------------------ the checks
class Job:
    def __init__(self, c, sort, res, worst):
        self.c, self.sort, self.cid, self.res, self.worst, self.fails, self.text = c, sort, kc.case_id(c), res, worst, [], []
        self.B, self.N = c[2], c[3]
        self.P = self.B * self.N
        self.f = ref_forward(c)
        self.ok_out, self.ok_grad = kc.exclusions(self.f)          # the rows compared strictly: outputs, gradients
        self.inside = self.f["in_img"].reshape(self.P)

    def fail(self, text):
        self.fails.append("%s: %s" % (self.cid, text))

    def take(self, name, shape, sentinel=SENTINEL):
        """an output out of its margins, which must be untouched"""
        buf = self.res["%s|%s" % (self.cid, name)]
        n = int(np.prod(shape))
        edge = np.concatenate([buf[:MARGIN], buf[MARGIN + n:]])
        if len(edge) != 2 * MARGIN or not (edge == sentinel).all():
            self.fail("wrote outside %s (%d margin elements changed)" % (name, int((edge != sentinel).sum())))
        return buf[MARGIN:MARGIN + n].reshape(shape)

    def pages(self):
        pg = self.res[self.cid + "|pages"]
        if not (pg == PAGE_BYTE).all():
            self.fail("wrote outside its staging or workspace (%d bytes of the sentinel pages changed)" % int((pg != PAGE_BYTE).sum()))

    def rows(self, a):
        """(B, C, N) -> (P, C)"""
        return a.reshape(self.B, -1, self.N).transpose(0, 2, 1).reshape(self.P, -1)

    def close(self, what, got, ref, ok, bound, floor_one):
        """got, ref (P, ...) rows per point: finite everywhere, and within bound * scale on the rows `ok`"""
        got, ref = got.reshape(self.P, -1).astype(np.float64), ref.reshape(self.P, -1)
        if not np.isfinite(got).all():
            self.fail("%s: %d entries not written or not finite" % (what, int((~np.isfinite(got)).sum())))
            return
        q = what.split("/")[-1]
        bound = kc.FLOORS.get((self.cid, q), (None, bound))[1]
        scale = max(1.0, np.abs(ref).max()) if floor_one else np.abs(ref).max()
        if not ok.any() or scale == 0:
            if np.abs(ref).max() == 0 and got.any():
                self.fail("%s is not 0" % what)
            return
        err = np.abs(got - ref)[ok]
        e = float(err.max() / scale)
        w = self.worst.setdefault((kc.OP_NAMES[self.c[0]], q), [0.0, 0.0, ""])
        if e / bound > w[0] / max(w[1], 1e-30):
            w[:] = [e, bound, self.cid]
        self.text.append("%s %.2e" % (q, e))
        if not e <= bound:
            per = err.max(1)
            p = int(np.flatnonzero(ok)[per.argmax()])
            self.fail("%s: error %.3e of the scale %.3e, bound %.3e, at %d of %d points, worst at point (%d, %d)" %
                      (what, e, scale, bound, int((per > bound * scale).sum()), len(per), p // self.N, p % self.N))

    def outputs(self, tag=""):
        """the four outputs and the masks of a forward"""
        f, got = self.f, {}
        for i, nm in zip(API_ORDER, ("df", "pca", "parts", "centers")):
            got[nm] = self.take(tag + nm, (self.B, OUT_DIM[i], self.N))
            self.close(tag + nm, self.rows(got[nm]), self.rows(f[nm]), self.ok_out, kc.OUT_BOUND, True)
        got["in_img"] = self.take(tag + "in_img", (self.B, self.N), PAGE_BYTE)
        away = f["border"] >= kc.BORDER_MIN
        if not np.array_equal(got["in_img"].reshape(self.P)[away], self.inside[away].astype(np.uint8)):
            self.fail("in_img differs from the reference's away from the border")
        filled = self.rows(got["df"]) == np.float32(qr.OUT_DIST)
        if not np.array_equal(filled[away], np.repeat(~self.inside[away, None], 2, 1)):
            self.fail("the df == 5.0 mask differs from the reference's away from the border")
        return got

    def staging(self, parts, back=None):
        f, P = self.f, self.P
        self.pages()
        for nm in parts:
            a = self.res["%s|%s" % (self.cid, nm)]
            if nm == "X":
                a, x32 = a.reshape(P, qr.KPAD), f["X32"]
                ne = (a + np.float32(0)).view(np.uint32) != (x32 + np.float32(0)).view(np.uint32)
                if ne.any():
                    p, ch = np.argwhere(ne)[0]
                    self.fail("X: %d of %d entries differ from the float32 restatement, first at point (%d, %d) channel %d: %r instead of %r" %
                              (int(ne.sum()), a.size, p // self.N, p % self.N, ch, float(a[p, ch]), float(x32[p, ch])))
                self.close("X", a, f["X"], self.ok_out, kc.OUT_BOUND, True)
            elif nm == "dX":
                self.close("dX", a.reshape(P, qr.KPAD), back["dX"], self.ok_grad, kc.GRAD_BOUND, False)
            else:
                a = a.reshape(3, 4, P, qr.HID).transpose(2, 0, 1, 3)              # rows per point
                ref = np.stack([np.stack(r) for r in (f["H"] if nm == "H" else back["dZ"])]).transpose(2, 0, 1, 3)
                self.close(nm, a, ref, self.ok_out if nm == "H" else self.ok_grad, kc.OUT_BOUND if nm == "H" else kc.GRAD_BOUND, nm == "H")
                if nm == "H" and np.isfinite(a).all() and not np.array_equal((a > 0)[self.ok_out], (ref > 0)[self.ok_out]):
                    self.fail("H: %d entries are zero on one side only where the ReLU margin holds" % int(((a > 0) != (ref > 0))[self.ok_out].sum()))


def check_fwd(j):
    got = j.outputs()
    if j.c[7] & qc.WS:
        j.pages()
        perm = j.res[j.cid + "|perm"].reshape(j.B, j.N)
        if j.sort and not all(np.array_equal(np.sort(p), np.arange(j.N)) for p in perm):
            j.fail("the workspace does not hold a permutation of 0..N-1")
        plain = j.outputs("plain/")
        for nm in got:
            if got[nm].tobytes() != plain[nm].tobytes():
                j.fail("%s differs from the call without a workspace" % nm)


def check_fwd_train(j):
    j.outputs()
    j.staging(("X", "H"))


def check_bwd_points(j):
    g = kc.grads_of(j.c)
    back = qr.backward(j.f, g)
    dp = j.take("dpoints", (j.P, 3))
    j.close("dpoints", dp, back["dpoints"], j.ok_grad, kc.GRAD_BOUND, False)
    away = (j.f["border"] >= kc.BORDER_MIN) & ~j.inside
    if j.c[6] == 1 and dp[away].any():
        j.fail("a gradient of df alone is not exactly 0 at %d points outside the image" % int(dp[away].any(1).sum()))


def check_surface_step(j):
    pts = j.f["points"].reshape(j.P, 3)
    for k, thr in enumerate(thresholds(j.c)):
        ref, clamp = qr.surface_step(j.f, k, thr)
        got = j.take("step%d" % k, (j.P, 3))
        ok = j.ok_grad & ~(clamp < kc.CLAMP_MIN)
        j.close("step%d" % k, got.astype(np.float64) - pts, ref.reshape(j.P, 3) - pts, ok, kc.GRAD_BOUND, False)
        away = (j.f["border"] >= kc.BORDER_MIN) & ~j.inside
        if not np.array_equal(got[away], pts[away].astype(np.float32)):
            j.fail("step %d moves points outside the image" % k)


def check_bwd_train(j):
    g = kc.grads_of(j.c)
    back = qr.backward(j.f, g)
    j.close("dpoints", j.take("dpoints", (j.P, 3)), back["dpoints"], j.ok_grad, kc.GRAD_BOUND, False)
    j.staging(("X", "H", "dZ", "dX"), back)


CHECKS = {qc.FWD: check_fwd, qc.FWD_TRAIN: check_fwd_train, qc.BWD_POINTS: check_bwd_points, qc.SURFACE_STEP: check_surface_step,
          qc.BWD_TRAIN: check_bwd_train}
SETS = [s[0] for s in qc.SWITCH_SETS]


@pytest.mark.parametrize("k", range(len(qc.SWITCH_SETS)), ids=SETS)
def test_switch_set(tmp_path, k):
    jobs = kc.jobs_of(k)
    print("switch set %s %s: %d calls" % (SETS[k], qc.SWITCH_SETS[k][2], len(jobs)))
    res, path = run_child(tmp_path, k)
    fails, worst = [], {}
    try:
        for c, name, sort in jobs:
            j = Job(c, sort, res, worst)
            CHECKS[c[0]](j)
            fails += j.fails
            print("  %-44s %-72s %s%s" % (j.cid, ("sort + " if sort else "") + name, " ".join(j.text), "  FAILED" if j.fails else ""))
    finally:
        res.close()
        os.remove(path)
    print("switch set %s: largest error per operation and quantity (error, bound, case)" % SETS[k])
    for (op, q), (e, b, cid) in sorted(worst.items()):
        print("  %-13s %-8s %.2e (%.1e)  %s" % (op, q, e, b, cid))
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails[:40])


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "--child":
    sys.path.insert(0, REPO)
    child_main(*sys.argv[2:5])
