"""GPU: the ConvBlock training operator, chore_convblock_fwd / chore_convblock_bwd (csrc/convblock.hip), stage by stage against
the float64 reference of tests/convblock_ref.py, in the three modes training uses (fp32, bf16, fp16 x 3).

What the block does that no per-layer entry point does, and what therefore only this module compares with anything: outputs
written at a channel offset with stride Cout next to a second `raw` output, a residual read through a strided view (for
Cin != Cout from y itself while y is written), two statistics accumulators per launch, the multi-job pack launch that clears
them; in the backward data gradients whose input is a channel slice of dy, weight gradients with a strided dy and one deferred
finish, GroupNorm backward with a strided skip gradient and a range output, the range of dy from the pack launch, all on two
streams joined by events.

Cases, switch sets, the `saved` layout and the pinned plan of every launch: tests/convblock_cases.py.  The library reads its
switches once per process, so each switch set runs in one child process (this file with --child, tests/gpu_child.py); inputs are
made on the CPU from a seed derived from the case id and handed over in an .npz, so device and reference see the same bits.
Calls go straight through the C API.

ReLU kinks.  A pre-activation within rounding of 0 takes another branch on the device than in float64.  Instead of masking, stored
INPUTS are moved (convblock_ref.nudge, KINK = 1e-3): x on the CPU before the run under bn1 / bn4; o1 and o2 between forward and
backward, in `saved` on the device, under bn2 / bn3 with the float64 statistics of the stored tensors -- the statistics cells stay
as the forward left them, so bn2 / bn3 normalise the nudged tensors with the statistics of the stored ones, and so does the reference
(on a 35-pixel map with one channel per group one moved element shifts a fresh mean by 1e-4 of the spread: 2.3e-5 in dW3).  At most 0.5 % of a tensor may move (asserted; 0.05 - 0.36 % of x do, 0.05 - 0.18 % of o1 / o2), and nothing is excluded from any comparison.

Forward, every job (the reference of each stage is fed what the device stored, so each quantity is one layer deep):
  a. the statistics cells of x, o1, o2, y against float64 group sums of the stored tensors, 2e-6
  b. o1, o2 and the third slice of y against their stage, the first two slices of y against o_k + res: fp32 / fp16 x 3 within 2e-5 of
     the reference's largest entry, bf16 within 3e-2 and 1.5e-2 relative L2; for Cin != Cout the residual is formed in float64 and
     the bound on y doubles (two layers' errors add)
  c. Cin == Cout, fp32 and fp16 x 3: the first two slices of y equal float32(o_k + x) bit for bit
  d. y between sentinel margins, pre-filled with NaN; `saved` and the workspace exactly their *_bytes plus a sentinel page, the
     workspace full of NaN garbage; chore_convblock_saved_bytes against the restated layout
  e. x_stats given (chore_gn_stats of x): every output bit-identical to the NULL run; a second identical call: identical bits
  f. chore_debug_last_conv equals the pinned row of conv3, the counter moved by 3 or 4
Backward, every job:
  g. dx and every parameter gradient against convblock_ref.backward on (x, nudged o1, nudged o2, dy): fp32 / fp16 x 3 within
     depth x 2e-5 of the reference's largest entry (convblock_cases.DEPTH: chained operators between dy and the output); bf16 within
     4 x (max) and 2 x (relative L2) the error of the storage rounding model against float64, which must itself stay below
     depth x (3e-2, 1.5e-2)
  h. dy variants on the tiny and ragged shapes: dy == 0 gives exact zeros everywhere; dy in one slice only gives exact zeros in the
     gradients that slice cannot reach and the bounds of g. elsewhere; the third slice at 2^-12 of the others (one range for the whole
     of dy): dW3 within its bound relative to its OWN largest entry
  i. guards as in d. on dx and the gradient arena; repeat and x_stats-given calls bit-identical
  j. chore_debug_last_conv equals the pinned row of the last data gradient (counter + 3 or 4), chore_debug_last_wgrad names the
     kernel wgrad_plan picks for conv1's weight gradient (counter + 3 or 4)
Across processes: CHORE_CONVBLOCK_SERIAL=1 (one stream) and CHORE_LDS_POISON give the bits of the default run; every refused
shape returns CHORE_EINVAL before any launch, and a legal call after them reproduces the default run's bits.

Measured on an MI355X (worst max error of the reference's largest entry / worst relative L2 over all 12 switch sets, 257 jobs;
next to the bound on the maximum).  The module takes 92 s, 33 tests: the default child 7 s, every other child 3 - 5 s, the rest is
float64 on the CPU; no test above 8.3 s.  The whole GPU suite took 630 s with it (1498 tests), 538 s without.
  output (depth)         fp32                   fp16 x 3               bound      bf16 (bounds: 4 x / 2 x the storage model's error)
  statistics x o1 o2 y   1.5e-07                1.5e-07                2e-6       9.0e-08
  o1, o2                 1.6e-06 / 6.2e-07      1.6e-06 / 5.5e-07      2e-5       4.0e-03 / 3.1e-03   (3e-2 / 1.5e-2)
  y                      6.4e-07 / 2.6e-07      5.9e-07 / 2.4e-07      2e-5, 4e-5 5.3e-03 / 3.2e-03   (3e-2 / 1.5e-2, twice that for Cin != Cout)
  dW3, dWd (1)           3.0e-07 / 2.2e-07      5.3e-07 / 3.3e-07      2e-5       2.7e-03 / 1.8e-03
  dgamma, dbeta 3, 4 (2) 7.2e-07 / 5.9e-07      1.4e-06 / 1.9e-06      4e-5       3.8e-03 / 3.4e-03
  dW2 (3)                9.1e-07 / 6.7e-07      9.6e-07 / 6.3e-07      6e-5       1.4e-02 / 1.2e-02
  dgamma2, dbeta2 (4)    1.3e-06 / 9.6e-07      2.5e-06 / 2.2e-06      8e-5       2.0e-02 / 1.6e-02
  dW1 (5)                8.1e-07 / 6.9e-07      8.1e-07 / 6.8e-07      1e-4       1.0e-02 / 1.3e-02
  dgamma1, dbeta1, dx (6) 1.4e-06 / 1.0e-06     2.1e-06 / 3.3e-06      1.2e-4     1.8e-02 / 1.7e-02
  bf16: at worst 0.28 of its maximum bound and 0.51 of its L2 bound (0.50 = the model's own error: the kernels are as exact as the
  number format allows); the model's bounds stayed below depth x (3e-2, 1.5e-2) everywhere (largest: 1x128x128, 128 -> 256).
  the third slice of dy at 2^-12 of the others: dW3 2.2e-07 (fp32) / 2.7e-07 (fp16 x 3) of its own largest entry, dgamma3 / dbeta3
  6.2e-07 / 5.9e-07 -- these two were 4.5e-03 / 4.8e-03 in fp32 and fp16 x 3 before the GroupNorm backward's accumulators got their own
  unit (train_bwd.hip, grad_add): the finding of this case.
  nudged: 0.05 - 0.18 % of o1 / o2 (cap 0.5 %).  Every exact-zero, bit-exact, repeat, x_stats, serial, poisoned-LDS, guard, page,
  witness and refusal check held.
"""
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref               # noqa: E402
import convblock_cases as bc  # noqa: E402
import convblock_ref as br    # noqa: E402
import gpu_child              # noqa: E402
from gpu_guards import PAGE_BYTE, SENTINEL, Guarded, Workspace  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_DT = {"fp32": torch.float32, "x3": torch.float32, "bf16": torch.bfloat16}
MARGIN = 256
CHILD_TIMEOUT = 600
EINVAL = -1
REFUSE_BYTES = 1 << 20
FLAGS = ("fwd workspace page", "x_stats given: identical bits", "forward repeat: identical bits", "saved page", "bwd workspace page",
         "backward repeat: identical bits", "backward x_stats given: identical bits", "chore_convblock_saved_bytes is the restated layout",
         "chore_convblock_grad_floats is the restated arena", "chore_convblock_out_stats_offset is three blocks")


def _strip(name):
    return name.startswith("CHORE_CONV") or name.startswith("CHORE_WGRAD") or name in ("CHORE_NO_CONV_SMALL", "CHORE_PC_FORCE", "CHORE_LDS_POISON")


RUNNER = gpu_child.ChildRunner(__file__, _strip)


def storage(mode):
    return "fp32" if mode == "x3" else mode


# ------------------------------------------------------------------------------------------------ inputs
_INPUTS = {}


def inputs_of(case):
    """-> dict: params, dy (float32), x per storage type (stored values as float32, kinks nudged away), nudged shares"""
    if case["id"] not in _INPUTS:
        x, p, dy = br.make_inputs(case)
        d = dict(p=p, dy=dy)
        for st in ("fp32", "bf16"):
            xs, moved, rounds = br.nudge(conv_ref.as_stored(x, st), br.x_norms(p), bc.KINK)
            assert moved.mean() <= bc.NUDGE_CAP, (case["id"], st, moved.mean())
            d["x." + st] = xs
        _INPUTS[case["id"]] = d
    return _INPUTS[case["id"]]


def arrays_of(jobs):
    out = {}
    for case, mode in jobs:
        d, cid = inputs_of(case), case["id"]
        out[cid + "/x." + storage(mode)] = d["x." + storage(mode)].float().numpy()
        out[cid + "/dy"] = d["dy"]
        for k, v in d["p"].items():
            out[cid + "/" + k] = v
    return out


# ------------------------------------------------------------------------------------------------ the child process
def _ibits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.dtype == torch.bfloat16 else t)


def _raw(t):
    return _ibits(t).cpu().numpy()


class _Dev:
    def __init__(self):
        from chore_amd import _lib
        self._lib, self.L, self.h = _lib, _lib.lib, _lib.handle(0)
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.code = {"fp32": _lib.F32, "bf16": _lib.BF16, "x3": _lib.F16X3}

    def last(self, which):
        rec = (ctypes.c_int * 8)()
        assert getattr(self.L, "chore_debug_last_" + which)(self.h, rec, 8) == 8
        return np.array(list(rec), np.int64)


def _job_tensors(D, data, case, mode):
    cid, tdt = case["id"], TORCH_DT[mode]
    x = torch.from_numpy(data[cid + "/x." + storage(mode)]).to(tdt).to(D.dev).contiguous()
    names = ["w1", "w2", "w3", "g1", "b1", "g2", "b2", "g3", "b3"] + (["wd", "g4", "b4"] if case["cin"] != case["cout"] else [])
    p = {k: torch.from_numpy(data[cid + "/" + k]).to(D.dev).contiguous() for k in names}
    gb = (ctypes.c_void_p * 8)(*[p[k].data_ptr() if k in p else None for k in ("g1", "b1", "g2", "b2", "g3", "b3", "g4", "b4")])
    return x, p, gb


def _fwd(D, case, mode, x, st, p, gb, y, saved, ws):
    c = case
    return D.L.chore_convblock_fwd(D.h, D.code[mode], x.data_ptr(), st, c["B"], c["H"], c["W"], c["cin"], c["cout"], p["w1"].data_ptr(),
                                   p["w2"].data_ptr(), p["w3"].data_ptr(), p["wd"].data_ptr() if "wd" in p else None, gb, y, saved, ws, D.stream)


def _bwd(D, case, mode, x, st, dy, p, gb, saved, dx, grads, ws):
    c = case
    return D.L.chore_convblock_bwd(D.h, D.code[mode], x.data_ptr(), st, dy.data_ptr(), c["B"], c["H"], c["W"], c["cin"], c["cout"],
                                   p["w1"].data_ptr(), p["w2"].data_ptr(), p["w3"].data_ptr(), p["wd"].data_ptr() if "wd" in p else None, gb,
                                   saved, dx, grads, ws, D.stream)


def run_job(D, data, case, mode, variants, out):
    """one job on the device -> its arrays into `out` under "<case>|<mode>|..." """
    L, dev, tdt, dt = D.L, D.dev, TORCH_DT[mode], D.code[mode]
    B, H, W, cin, cout = (case[k] for k in ("B", "H", "W", "cin", "cout"))
    c1, c2, px = cout // 2, cout // 4, B * H * W
    key = case["id"] + "|" + mode
    x, p, gb = _job_tensors(D, data, case, mode)
    lay = bc.saved_layout(mode, B, H, W, cout)
    _, nfloats = bc.grad_layout(cin, cout)
    nsaved, nws, nb = (L.chore_convblock_saved_bytes(dt, B, H, W, cin, cout), L.chore_convblock_workspace_bytes(dt, B, H, W, cin, cout),
                       L.chore_gn_stats_bytes(B))
    flags = {f: 1 for f in FLAGS}
    flags[FLAGS[7]] = int(nsaved == lay["bytes"] and nb == bc.stats_bytes(B))
    flags[FLAGS[8]] = int(L.chore_convblock_grad_floats(cin, cout) == nfloats)
    flags[FLAGS[9]] = int(L.chore_convblock_out_stats_offset(B) == lay["sy"])
    assert nsaved > 0 and nws > 0, key
    what = "convblock %s" % key

    def check(rc, text):
        D._lib.check(rc, D.h, "%s %s" % (text, key))

    def page_ok(w):
        return int((w.buf[w.nbytes:] == PAGE_BYTE).all().item())

    # ---- forward: statistics given, then NULL twice ----
    st = torch.zeros(nb, dtype=torch.uint8, device=dev)
    check(L.chore_gn_stats(D.h, D._lib.F32 if mode == "x3" else dt, x.data_ptr(), B, H * W, cin, st.data_ptr(), 1, D.stream), "gn_stats")
    runs = []
    for given in (True, False, False):
        y, saved, ws = Guarded(px * cout, dev, tdt, MARGIN), Workspace(nsaved, dev), Workspace(nws, dev)
        before = D.last("conv")[7]
        check(_fwd(D, case, mode, x, st.data_ptr() if given else None, p, gb, y.ptr, saved.ptr, ws.ptr), "fwd")
        torch.cuda.synchronize()
        rec = D.last("conv")
        flags[FLAGS[0]] &= page_ok(ws)
        flags[FLAGS[3]] &= page_ok(saved)
        runs.append((y, saved, rec, int(rec[7] - before)))
        del ws
    (ya, sa, _, _), (y, saved, rec_f, step_f), (yc, sc, _, _) = runs
    flags[FLAGS[1]] = int(torch.equal(_ibits(ya.buf), _ibits(y.buf)) and torch.equal(sa.buf[nb:], saved.buf[nb:]) and
                          torch.equal(saved.buf[:nb], st))
    flags[FLAGS[2]] = int(torch.equal(_ibits(yc.buf), _ibits(y.buf)) and torch.equal(sc.buf, saved.buf))
    del runs, ya, sa, yc, sc
    out[key + "|y"] = _raw(y.buf)
    out[key + "|saved"] = saved.buf.cpu().numpy()
    dig_f = hashlib.sha256(out[key + "|y"].tobytes() + out[key + "|saved"].tobytes()).digest()

    # ---- ReLU kinks of o1 / o2: nudged in `saved`, the statistics cells untouched ----
    host = saved.buf.cpu()
    for name, off, ch, g, b in (("o1", lay["o1"], c1, "g2", "b2"), ("o2", lay["o2"], c2, "g3", "b3")):
        nbytes = px * ch * bc.ELEM_BYTES[mode]
        t = host[off:off + nbytes].view(tdt).reshape(B, H, W, ch)
        new, moved, _ = br.nudge(t, [(p[g].cpu().numpy(), p[b].cpu().numpy())], bc.KINK, br.group_stats(t))
        idx = np.flatnonzero(moved.reshape(-1))
        vals = new.reshape(-1)[torch.from_numpy(idx)]
        if idx.size:
            saved.buf[off:off + nbytes].view(tdt)[torch.from_numpy(idx).to(dev)] = vals.to(dev)
        out[key + "|%s.idx" % name], out[key + "|%s.val" % name] = idx, vals.float().numpy()

    # ---- backward ----
    def backward(dy_np, given=False):
        dy = torch.from_numpy(dy_np).to(tdt).to(dev).contiguous()
        dx, grads, ws = Guarded(px * cin, dev, tdt, MARGIN), Guarded(nfloats, dev, torch.float32, MARGIN), Workspace(nws, dev)
        bc_, bw_ = D.last("conv")[7], D.last("wgrad")[7]
        check(_bwd(D, case, mode, x, st.data_ptr() if given else None, dy, p, gb, saved.ptr, dx.ptr, grads.ptr, ws.ptr), "bwd")
        torch.cuda.synchronize()
        rc_, rw_ = D.last("conv"), D.last("wgrad")
        flags[FLAGS[4]] &= page_ok(ws)
        flags[FLAGS[3]] &= page_ok(saved)
        return dx, grads, rc_, int(rc_[7] - bc_), rw_, int(rw_[7] - bw_)

    dy_main = data[case["id"] + "/dy"]
    dx, grads, rec_b, step_b, rec_w, step_w = backward(dy_main)
    for given, flag in ((False, FLAGS[5]), (True, FLAGS[6])):
        dx2, grads2 = backward(dy_main, given)[:2]
        flags[flag] = int(torch.equal(_ibits(dx2.buf), _ibits(dx.buf)) and torch.equal(_ibits(grads2.buf), _ibits(grads.buf)))
        del dx2, grads2
    out[key + "|dx"], out[key + "|grads"] = _raw(dx.buf), _raw(grads.buf)
    hb = hashlib.sha256(out[key + "|dx"].tobytes() + out[key + "|grads"].tobytes())
    if variants:
        for name, v in bc.VARIANTS.items():
            vdx, vgr = backward(br.variant_dy(dy_main, cout, v))[:2]
            out[key + "|%s|dx" % name], out[key + "|%s|grads" % name] = _raw(vdx.buf), _raw(vgr.buf)
            hb.update(out[key + "|%s|dx" % name].tobytes() + out[key + "|%s|grads" % name].tobytes())
    out[key + "|digest"] = np.frombuffer(dig_f + hb.digest(), np.uint8).reshape(2, 32)
    out[key + "|flags"] = np.array([flags[f] for f in FLAGS], np.int64)
    out[key + "|recs"] = np.stack([np.append(rec_f, step_f), np.append(rec_b, step_b), np.append(rec_w, step_w)])


def run_refusals(D, out):
    """every row of convblock_cases.REFUSED, forward and backward: the return code, the text, both launch counters, every buffer"""
    L, dev = D.L, D.dev
    rows = []
    for what, dt, B, cin, cout, wd_given, text in bc.REFUSED:
        for call in ("fwd", "bwd"):
            bufs = [Guarded(REFUSE_BYTES // 4, dev, fill=3.0) for _ in range(5)]         # y / dx, saved, workspace, grads, spare
            x = torch.zeros(REFUSE_BYTES // 4, device=dev)
            w = torch.zeros(9 * 256 * 256, device=dev)
            gbt = torch.ones(512, device=dev)
            gb = (ctypes.c_void_p * 8)(*[gbt.data_ptr()] * 8)
            wd = w.data_ptr() if wd_given else None
            before = (int(D.last("conv")[7]), int(D.last("wgrad")[7]))
            if call == "fwd":
                rc = L.chore_convblock_fwd(D.h, dt, x.data_ptr(), None, B, 5, 7, cin, cout, w.data_ptr(), w.data_ptr(), w.data_ptr(), wd, gb,
                                           bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, D.stream)
            else:
                rc = L.chore_convblock_bwd(D.h, dt, x.data_ptr(), None, x.data_ptr(), B, 5, 7, cin, cout, w.data_ptr(), w.data_ptr(), w.data_ptr(),
                                           wd, gb, bufs[1].ptr, bufs[0].ptr, bufs[3].ptr, bufs[2].ptr, D.stream)
            msg = L.chore_last_error(D.h).decode()
            torch.cuda.synchronize()
            after = (int(D.last("conv")[7]), int(D.last("wgrad")[7]))
            clean = all(bool((b.buf[b.m:b.m + b.n] == 3.0).all().item()) and bool((b.buf[:b.m] == SENTINEL).all().item()) and
                        bool((b.buf[b.m + b.n:] == SENTINEL).all().item()) for b in bufs)
            rows.append(dict(what=what, call=call, rc=int(rc), msg=msg, text=text, counters=before == after, clean=clean))
    out["refusals"] = np.frombuffer(json.dumps(rows).encode(), np.uint8)


def child_main(in_path, job_path, out_path):
    jobs = json.load(open(job_path))
    data = np.load(in_path)
    D = _Dev()
    out = {}
    for job in jobs:
        if job[0] == "refusals":
            run_refusals(D, out)
        else:
            run_job(D, data, bc.CASES[job[0]], job[1], bool(job[2]), out)
    np.savez(out_path, **out)


# ------------------------------------------------------------------------------------------------ the checks
WORST = {}          # (mode, output) -> [max error / its bound basis, relative L2, where]


def _note(mode, name, emax, el2, where):
    w = WORST.setdefault((mode, name), [0.0, 0.0, ""])
    if emax > w[0]:
        w[0], w[2] = emax, where
    w[1] = max(w[1], el2)


def _close(fails, got, ref, what, mode, name, bmax, bl2=None, top=None):
    if not np.isfinite(got).all():
        fails.append("%s: %d entries not written or not finite, first at %s" % (what, int((~np.isfinite(got)).sum()),
                                                                               tuple(int(v) for v in np.argwhere(~np.isfinite(got))[0])))
        return
    top = np.abs(ref).max() if top is None else top
    assert top > 0, what
    emax = float(np.abs(got - ref).max() / top)
    el2 = float(np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel()))
    _note(mode, name, emax, el2, what)
    if not emax <= bmax:
        fails.append("%s: max error %.3e of the largest entry, bound %.3e, at %s" % (
            what, emax, bmax, tuple(int(v) for v in np.unravel_index(np.abs(got - ref).argmax(), ref.shape))))
    if bl2 is not None and not el2 <= bl2:
        fails.append("%s: relative L2 error %.3e, bound %.3e" % (what, el2, bl2))
    return emax, el2


def _unguard(raw, n, mode, what, fails, f32=False):
    """the payload of a guarded buffer as the stored torch tensor; the margins must hold the sentinel"""
    tdt = torch.float32 if f32 else TORCH_DT[mode]
    t = torch.from_numpy(raw).view(tdt)
    if not (bool((t[:MARGIN] == SENTINEL).all()) and bool((t[MARGIN + n:] == SENTINEL).all())):
        fails.append("%s: wrote outside its output" % what)
    return t[MARGIN:MARGIN + n]


def _stored(t, off, shape, mode):
    n = int(np.prod(shape)) * bc.ELEM_BYTES[mode]
    return torch.from_numpy(t[off:off + n].copy()).view(TORCH_DT[mode]).reshape(shape)


def _split_grads(g, case):
    lay, _ = bc.grad_layout(case["cin"], case["cout"])
    return {k: g[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in lay.items()}


_STAGE1 = {}        # (case, storage) -> (conv1's reference, the residual in float64)


def check_job(set_name, case, mode, res, variants):
    """-> list of failure texts"""
    cid = case["id"]
    key = cid + "|" + mode
    B, H, W, cin, cout = (case[k] for k in ("B", "H", "W", "cin", "cout"))
    c1, c2, px = cout // 2, cout // 4, B * H * W
    st = storage(mode)
    inp = inputs_of(case)
    p, xs = inp["p"], inp["x." + st]
    fails = []
    tag = "%s %s %s" % (set_name, cid, mode)
    bmax, bl2 = bc.LAYER_BOUNDS[mode]
    # d. e. guards, pages, repeats, the size functions
    for f, ok in zip(FLAGS, res[key + "|flags"]):
        if not ok:
            fails.append("%s: failed: %s" % (tag, f))
    # f. j. the witnesses
    rec_f, rec_b, rec_w = res[key + "|recs"]
    plan = bc.plan_of(set_name, case, mode)
    nconv = 4 if cin != cout else 3
    if tuple(rec_f[:6]) != plan[nconv - 1] or rec_f[6] != c2 or rec_f[8] != nconv:
        fails.append("%s: forward witness %s, pinned %s with %d input channels, %d launches" % (tag, list(rec_f), plan[nconv - 1], c2, nconv))
    if tuple(rec_b[:6]) != plan[-1] or rec_b[6] != c1 or rec_b[8] != nconv:
        fails.append("%s: backward witness %s, pinned %s with %d input channels, %d launches" % (tag, list(rec_b), plan[-1], c1, nconv))
    wk = bc.wgrad_kernel(mode, 9, B, H, W, cin, c1, bc.SWITCH_SETS[set_name][0])
    if tuple(rec_w[:3]) != wk + (9,) or not rec_w[6] & 1 or rec_w[8] != nconv:
        fails.append("%s: weight-gradient witness %s, expected kernel %s taps 9 with GroupNorm, %d launches" % (tag, list(rec_w), wk, nconv))
    # ---- forward ----
    lay = bc.saved_layout(mode, B, H, W, cout)
    saved = res[key + "|saved"]
    y = _unguard(res[key + "|y"], px * cout, mode, tag + " y", fails).reshape(B, H, W, cout)
    o1, o2 = _stored(saved, lay["o1"], (B, H, W, c1), mode), _stored(saved, lay["o2"], (B, H, W, c2), mode)
    y64, o1_64, o2_64, x64 = y.double().numpy(), o1.double().numpy(), o2.double().numpy(), xs.double().numpy()
    if not (np.isfinite(y64).all() and np.isfinite(o1_64).all() and np.isfinite(o2_64).all()):
        fails.append("%s: y / o1 / o2 hold entries not written or not finite (%d / %d / %d)" % (
            tag, int((~np.isfinite(y64)).sum()), int((~np.isfinite(o1_64)).sum()), int((~np.isfinite(o2_64)).sum())))
        return fails
    # a. statistics
    nb = bc.stats_bytes(B)
    for name, off, t in (("x", lay["sx"], x64), ("o1", lay["s1"], o1_64), ("o2", lay["s2"], o2_64), ("y", lay["sy"], y64)):
        got, want = conv_ref.stat_values(saved[off:off + nb].copy().view(np.int64)), conv_ref.group_sums(t)
        es = float(np.abs(got - want).max() / np.abs(want).max())
        _note(mode, "stats " + name, es, 0.0, tag)
        if not es <= bc.STAT_TOL:
            fails.append("%s: statistics of %s off by %.3e relative, bound %.0e" % (tag, name, es, bc.STAT_TOL))
    # b. values
    if (cid, st) not in _STAGE1:
        _STAGE1[(cid, st)] = (br.stage(xs, p["w1"], p["g1"], p["b1"]), br.stage(xs, p["wd"], p["g4"], p["b4"]) if cin != cout else x64)
    r1, res64 = _STAGE1[(cid, st)]
    r2 = br.stage(o1, p["w2"], p["g2"], p["b2"])
    r3 = br.stage(o2, p["w3"], p["g3"], p["b3"])
    _close(fails, o1_64, r1, tag + " o1", mode, "o1", bmax, bl2)
    _close(fails, o2_64, r2, tag + " o2", mode, "o2", bmax, bl2)
    k = 2 if cin != cout else 1
    yb, yl = k * bmax, (k * bl2 if bl2 else None)
    sl = ((0, c1), (c1, c1 + c2), (c1 + c2, cout))
    for i, (ref_o, (lo, hi)) in enumerate(zip((o1_64, o2_64, r3), sl)):
        _close(fails, y64[..., lo:hi], ref_o + res64[..., lo:hi], tag + " y slice %d" % (i + 1), mode, "y", yb, yl)
    # c. the epilogue stores raw = acc and out = acc + res
    if cin == cout and mode != "bf16":
        for i, (o, (lo, hi)) in enumerate(zip((o1, o2), sl[:2])):
            want = o.numpy() + xs[..., lo:hi].numpy()
            ne = want.view(np.uint32) != np.ascontiguousarray(y[..., lo:hi].numpy()).view(np.uint32)
            if ne.any():
                fails.append("%s: y slice %d is not float32(o%d + x) bit for bit: %d of %d entries, first at %s" % (
                    tag, i + 1, i + 1, int(ne.sum()), ne.size, tuple(int(v) for v in np.argwhere(ne)[0])))
    # ---- backward ----
    nud, frozen = {}, {"o1": br.group_stats(o1), "o2": br.group_stats(o2)}      # the statistics stay those of the stored tensors
    for name, t in (("o1", o1), ("o2", o2)):
        idx, val = res[key + "|%s.idx" % name], res[key + "|%s.val" % name]
        share = idx.size / t.numel()
        _note(mode, "nudged " + name, share, 0.0, tag)
        if share > bc.NUDGE_CAP:
            fails.append("%s: %.3f %% of %s nudged, cap %.2f %%" % (tag, 100 * share, name, 100 * bc.NUDGE_CAP))
        t = t.clone()
        t.view(-1)[torch.from_numpy(idx)] = torch.from_numpy(val).to(t.dtype)
        nud[name] = t
        assert br.kinks(t, [(p["g2"], p["b2"]) if name == "o1" else (p["g3"], p["b3"])], bc.KINK, frozen[name]) == 0
    runs = [("", inp["dy"], None)] + ([(n, br.variant_dy(inp["dy"], cout, v), n) for n, v in bc.VARIANTS.items()] if variants else [])
    for name, dy_np, variant in runs:
        pre = key + ("|%s" % name if name else "")
        vt = tag + (" dy %s" % name if name else "")
        dx = _unguard(res[pre + "|dx"], px * cin, mode, vt + " dx", fails).double().numpy().reshape(B, H, W, cin)
        got = _split_grads(_unguard(res[pre + "|grads"], bc.grad_layout(cin, cout)[1], mode, vt + " grads", fails, f32=True).double().numpy(), case)
        got["dx"] = dx
        bad = [k for k, v in got.items() if not np.isfinite(v).all()]
        if bad:
            fails.append("%s: entries not written or not finite in %s" % (vt, bad))
            continue
        if variant == "zero":
            nz = [k for k, v in got.items() if v.any()]
            if nz:
                fails.append("%s: not exactly zero: %s" % (vt, nz))
            continue
        dys = conv_ref.as_stored(dy_np, mode)
        ref = br.backward(xs, nud["o1"], nud["o2"], dys, p, None, frozen)
        model = br.backward(xs, nud["o1"], nud["o2"], dys, p, br.bf16_round, frozen) if mode == "bf16" else None
        zero = bc.EXACT_ZERO.get(variant, ())
        for k in sorted(got, key=lambda k: (bc.DEPTH[k], k)):
            d = bc.DEPTH[k]
            if k in zero:
                if got[k].any() or ref[k].any():
                    fails.append("%s: %s is not exactly zero (%d entries, reference %d)" % (vt, k, int((got[k] != 0).sum()), int((ref[k] != 0).sum())))
                continue
            if model is None:
                b1, b2 = d * bmax, None
            else:
                m, l2 = conv_ref.rel_max(model[k], ref[k]), conv_ref.rel_l2(model[k], ref[k])
                b1, b2 = bc.BF16_MODEL_MARGIN[0] * m, bc.BF16_MODEL_MARGIN[1] * l2
                if not (b1 < d * bmax and b2 < d * bl2):
                    fails.append("%s: %s: the bf16 model's bounds %.3e / %.3e are not below depth x (%.0e, %.0e)" % (vt, k, b1, b2, bmax, bl2))
            e = _close(fails, got[k], ref[k], "%s %s" % (vt, k), mode, k + (" " + variant if variant else ""), b1, b2)
            if e and model is not None:
                _note(mode, k + " / bound", e[0] / b1, e[1] / b2, vt)
    return fails


_RESULTS = {}      # switch set -> (failures per case id, digests), or the text of why its child gave no result
_FILES = []


@pytest.fixture(scope="module")
def outdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("convblock")
    yield d
    for r, path in _FILES:
        r.close()
        if os.path.exists(path):
            os.remove(path)
    print("worst errors of the session, (mode, output): [max, relative L2, where]")
    for k in sorted(WORST):
        print("  %-6s %-22s max %.2e  L2 %.2e   %s" % (k[0], k[1], WORST[k][0], WORST[k][1], WORST[k][2]))


def run_set(name, outdir, env=None, jobs=None, tag=None):
    """the checked results of a switch set.  Its child runs once per session whatever becomes of it"""
    tag = tag or name
    if tag not in _RESULTS:
        jobs = bc.jobs_of(name) if jobs is None else jobs
        env = bc.SWITCH_SETS[name][0] if env is None else env
        check = name != "serial" and tag == name
        print("switch set %s %s: %d jobs" % (tag, env, len(jobs)))
        _RESULTS[tag] = "the child of switch set %s did not finish" % tag
        t0 = time.time()
        try:
            res, path = RUNNER.run(outdir, tag, env, arrays_of(jobs), [(c["id"], m, int(c["variants"] and name == "default")) for c, m in jobs],
                                   CHILD_TIMEOUT)
        except BaseException as ex:      # (pytest.fail's exception derives from BaseException)
            _RESULTS[tag] = "switch set %s gave no result: %s" % (tag, str(ex)[:2000])
            raise
        _FILES.append((res, path))
        print("switch set %s: child took %.1f s" % (tag, time.time() - t0))
        fails, digests = {}, {}
        for case, mode in jobs:
            digests[case["id"] + "|" + mode] = res[case["id"] + "|" + mode + "|digest"].copy()
            if check and name != "default":          # ("default": case by case, test_default)
                fails.setdefault(case["id"], []).extend(check_job(name, case, mode, res, False))
        _RESULTS[tag] = (fails, digests, res)
    if isinstance(_RESULTS[tag], str):
        pytest.fail(_RESULTS[tag], pytrace=False)
    return _RESULTS[tag]


def _report(fails):
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails[:40])


@pytest.mark.parametrize("cid", list(bc.CASES))
def test_default(outdir, cid):
    """one case in the three modes under default switches: every check of the module docstring, the dy variants where the case has them"""
    _, _, res = run_set("default", outdir)
    case, fails = bc.CASES[cid], []
    for mode in bc.MODES:
        fails += check_job("default", case, mode, res, case["variants"])
    _report(fails)


@pytest.mark.parametrize("name", [n for n in bc.SWITCH_SETS if n not in ("default", "serial")])
def test_switch_set(outdir, name):
    """the jobs whose plan the switch set changes: the same checks on the main dy"""
    fails, _, _ = run_set(name, outdir)
    _report([f for v in fails.values() for f in v])


def _same_digests(a, b, what):
    diff = ["%s %s" % (k, ("forward " if (a[k][0] != b[k][0]).any() else "") + ("backward" if (a[k][1] != b[k][1]).any() else ""))
            for k in b if (a[k] != b[k]).any()]
    assert not diff, "%s: %d jobs differ from the default run's bits:\n%s" % (what, len(diff), "\n".join(diff[:40]))


def test_serial_is_bit_identical(outdir):
    """CHORE_CONVBLOCK_SERIAL=1 puts the whole backward on one stream: every output of every job must equal the two-stream run's bit
    for bit -- the check of the side stream's events (forward, backward, every dy variant)"""
    _, dflt, _ = run_set("default", outdir)
    jobs = bc.jobs_of("serial")
    _, ser, _ = run_set("default", outdir, env=bc.SWITCH_SETS["serial"][0], jobs=jobs, tag="serial")
    assert len(ser) == len(dflt) == len(jobs)
    _same_digests(dflt, ser, "serial")


def test_no_uninitialised_lds_read(outdir):
    """one case per family in every mode with every CU's LDS poisoned after every launch: the default run's bits"""
    _, dflt, _ = run_set("default", outdir)
    jobs = [(bc.CASES[c], m) for c in bc.POISON_CASES for m in bc.MODES]
    _, poi, _ = run_set("default", outdir, env=bc.POISON_ENV, jobs=jobs, tag="poison")
    assert len(poi) == len(jobs)
    _same_digests(dflt, poi, "poisoned LDS")


def test_refusals(outdir):
    """every row of convblock_cases.REFUSED in both calls: CHORE_EINVAL with a text naming the channel count, both launch counters
    unchanged, every buffer untouched; then a legal call on the same handle reproduces the default run's bits"""
    _, dflt, _ = run_set("default", outdir)
    case = bc.CASES[bc.REFUSED_THEN]
    jobs = [(case, m) for m in bc.MODES]
    res, path = RUNNER.run(outdir, "refusals", {}, arrays_of(jobs), [("refusals",)] + [(case["id"], m, 1) for m in bc.MODES], CHILD_TIMEOUT)
    try:
        rows = json.loads(res["refusals"].tobytes().decode())
        assert len(rows) == 2 * len(bc.REFUSED)
        bad = [r for r in rows if r["rc"] != EINVAL or r["text"] not in r["msg"] or not r["counters"] or not r["clean"]]
        assert not bad, bad
        _same_digests(dflt, {c["id"] + "|" + m: res[c["id"] + "|" + m + "|digest"] for c, m in jobs}, "after the refused calls")
    finally:
        res.close()
        os.remove(path)


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "--child":
    sys.path.insert(0, REPO)
    child_main(*sys.argv[2:5])
