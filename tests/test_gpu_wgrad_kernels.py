"""GPU: every weight-gradient kernel behind chore_conv2d_bwd_weight (wgrad_kernel / wgrad64_kernel / wgrad64_x3_kernel /
wgrad64_x3_pc_kernel / wgrad128_x3_pc_kernel of csrc/train_bwd.hip, and the ordered finish) against the float64 reference of
tests/conv_ref.py (weight_gradient: autograd of conv2d(relu(group_norm(x)), w) + bias).

Cases (tests/wgrad_cases.py) go through chore_conv2d_bwd_weight.  The library reads its switches once per process, so every
switch set runs in a child process of its own (this file with --child, tests/gpu_child.py); the parent makes the inputs on the CPU
from a seed derived from the case id and hands them over in an .npz, so device and reference see the same bits, and a case's
reference is computed once per storage type and reused across the switch sets.  A child returns, per case and mode, the dW and
dbias buffers, the sentinel page behind the workspace and the chore_debug_last_wgrad record (which kernel the launch chose).

Checks per case
  a. values ("gn": x ~ 1.5 N(0,1) + 0.3 through GroupNorm, dy ~ N(0,1), in x3 mode times a power of ten from 1e-7 to 3e4 by the
     shape): dW and dbias of fp32 and fp16 x 3 within 2e-5 of the reference's largest entry; bf16 within 3e-2 of it and 1.5e-2
     relative L2, the reference fed the bf16-rounded x and dy (the bounds of test_gpu_train_ops.py).
  b. exact ("exact": no GroupNorm, x and dy in {-1, 0, 1}): dW and dbias equal the float64 result bit for bit in every mode (the
     sign of a zero aside): the x3 operand scale is a power of two and every partial sum an integer times it, far below 2^24
     steps.  A wrong tap, halo column, tile-edge pixel or share shows here; a mismatch is reported as (o, c, tap) with its
     position in the channel tile and the witness record.
  c. zero gradient ("zero": dy == 0, GroupNorm recomputed): dW and dbias exactly 0.
  d. guards: dW and dbias live inside sentinel margins, pre-filled with NaN, and must come back finite with the margins unchanged;
     the workspace is chore_conv2d_wgrad_workspace_bytes(...) of NaNs plus a sentinel page that must come back unchanged: the size
     function is checked against every kernel, the forced ones included, and no kernel may rely on a zeroed workspace.
  e. one more pair of children on one case per kernel, without and with CHORE_LDS_POISON: bit-identical results.
  f. coverage: every row of wgrad_cases.COVERAGE that is marked to-reach was reported by the witness for at least one case, and
     the witness reported nothing the table does not name.

Measured on an MI355X (worst of dW and dbias over the matrix, next to the bound):
  mode    worst max error (bound)      worst relative L2 (bound)    where
    fp32    9.4e-07 (2e-5)               5.5e-07                      default switches
    fp16x3  5.1e-07 (2e-5)               3.8e-07                      CHORE_WGRAD_X3_PC=1 / CHORE_WGRAD_X3_V1=1
    bf16    2.0e-03 (3e-2)               1.7e-03 (1.5e-2)             default switches
  the exact and the zero-gradient cases, the guard margins, the workspace page, the poisoned-LDS run and the coverage table (20 rows,
  18 to reach, 18 reached: wgrad64_x3_pc_kernel<9> under default switches, wgrad64_x3_kernel<1>, wgrad_kernel<bf16, 1> and both
  mappings of every 64- and 128-channel kernel among them) held in all 4 switch sets, 225 launches; the module takes 20 s.
"""
import ctypes
import json
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref              # noqa: E402
import gpu_child             # noqa: E402
import wgrad_cases as wc     # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 7.0
DW_MARGIN, DB_MARGIN, WS_PAGE = 1024, 64, 4096       # floats, floats, bytes
WS_BYTE = 0xA5
TORCH_DT = {"fp32": torch.float32, "x3": torch.float32, "bf16": torch.bfloat16}
BOUNDS = {"fp32": (2e-5, None), "x3": (2e-5, None), "bf16": (3e-2, 1.5e-2)}      # (max, relative L2) of the reference's largest entry
EXACT_MAX = 2 ** 24
CHILD_TIMEOUT = 300


def _strip(name):
    return name.startswith("CHORE_WGRAD") or name.startswith("CHORE_LDS_POISON")


RUNNER = gpu_child.ChildRunner(__file__, _strip)


# ------------------------------------------------------------------------------------------------ inputs and references
def make_inputs(case):
    """the tensors of a case as numpy arrays (NHWC); seed from the case id"""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    B, H, W, cin, cout = (case[k] for k in ("B", "H", "W", "cin", "cout"))
    d = {}
    if case["kind"] == "exact":
        d["x"] = rng.integers(-1, 2, (B, H, W, cin), dtype=np.int8)
        d["dy"] = rng.integers(-1, 2, (B, H, W, cout), dtype=np.int8)
        return d
    d["x"] = (rng.standard_normal((B, H, W, cin), dtype=np.float32) * 1.5 + 0.3).astype(np.float32)
    d["gamma"] = (rng.random(cin, dtype=np.float32) + 0.5).astype(np.float32)
    d["beta"] = (rng.standard_normal(cin, dtype=np.float32) * 0.2).astype(np.float32)
    if case["kind"] == "gn":
        d["dy"] = rng.standard_normal((B, H, W, cout), dtype=np.float32)
    return d                 # ("zero": the child makes dy itself)


def dy_of(case, mode, dy):
    """the upstream gradient the device is handed in `mode`, float32 numpy: scaled in x3 mode (the same float32 product in parent and child)"""
    dy = np.asarray(dy, dtype=np.float32)
    if mode == "x3" and case["kind"] == "gn":
        dy = dy * np.float32(case["x3_scale"])
    return dy


_INPUTS, _REFS = {}, {}


def inputs_of(case):
    if case["id"] not in _INPUTS:
        _INPUTS[case["id"]] = make_inputs(case)
    return _INPUTS[case["id"]]


def reference(case, mode):
    """(dW, dbias) in float64 as the mode's storage sees x and dy; computed once per (case, what the device is handed)"""
    if case["kind"] == "zero":
        return None
    key = (case["id"], "exact" if case["kind"] == "exact" else mode)
    if key not in _REFS:
        d = inputs_of(case)
        k = 3 if case["taps"] == 9 else 1
        xs = conv_ref.as_stored(np.asarray(d["x"], dtype=np.float32), mode)
        dys = conv_ref.as_stored(dy_of(case, mode, d["dy"]), mode)
        dw, db = conv_ref.weight_gradient(xs, dys, k, d.get("gamma"), d.get("beta"))
        if case["kind"] == "exact":
            for t in (dw, db):
                assert np.abs(t).max() < EXACT_MAX and np.array_equal(t, np.rint(t)), case["id"]
            assert np.abs(dw).max() > 0
        _REFS[key] = (dw, db)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ the child process
def child_main(in_path, job_path, out_path):
    from chore_amd import _lib
    jobs = json.load(open(job_path))
    data = np.load(in_path)
    dev = torch.device("cuda", 0)
    h = _lib.handle(0)
    L = _lib.lib
    stream = torch.cuda.current_stream().cuda_stream
    code = {"fp32": _lib.F32, "bf16": _lib.BF16, "x3": _lib.F16X3}
    cases = {c["id"]: c for c in wc.cases()}
    out = {}

    def last():
        rec = (ctypes.c_int * 8)()
        assert L.chore_debug_last_wgrad(h, rec, 8) == 8
        return np.array(list(rec), np.int64)

    def guarded(n, margin):
        buf = torch.full((n + 2 * margin,), SENTINEL, dtype=torch.float32, device=dev)
        buf[margin:margin + n] = float("nan")
        return buf, buf.data_ptr() + 4 * margin

    for cid, mode in jobs:
        c = cases[cid]
        B, H, W, cin, cout, taps = (c[k] for k in ("B", "H", "W", "cin", "cout", "taps"))
        dt, tdt = code[mode], TORCH_DT[mode]

        def get(name, t=torch.float32):
            key = cid + "/" + name
            return torch.from_numpy(data[key].astype(np.float32)).to(t).to(dev).contiguous() if key in data.files else None
        x, gamma, beta = get("x", tdt), get("gamma"), get("beta")
        if c["kind"] == "zero":
            dy = torch.zeros(B, H, W, cout, dtype=tdt, device=dev)
        else:
            dy = torch.from_numpy(dy_of(c, mode, data[cid + "/dy"])).to(tdt).to(dev).contiguous()
        st = None
        if gamma is not None:
            st = torch.zeros(L.chore_gn_stats_bytes(B), dtype=torch.uint8, device=dev)
            _lib.check(L.chore_gn_stats(h, dt, x.data_ptr(), B, H * W, cin, st.data_ptr(), 1, stream), h, "gn_stats")
        amax = None
        if mode == "x3":
            amax = torch.zeros(L.chore_amax_bytes(), dtype=torch.uint8, device=dev)
            _lib.check(L.chore_absmax_f32(h, dy.data_ptr(), dy.numel(), amax.data_ptr(), stream), h, "absmax")
        n = cout * cin * taps
        dwbuf, dw = guarded(n, DW_MARGIN)
        dbbuf, db = guarded(cout, DB_MARGIN) if c["bias"] else (None, None)
        nws = L.chore_conv2d_wgrad_workspace_bytes(taps, B, H, W, cin, cout)
        assert nws > 0 and nws % 4 == 0, (cid, nws)
        ws = torch.full((nws + WS_PAGE,), WS_BYTE, dtype=torch.uint8, device=dev)
        ws[:nws].view(torch.float32).fill_(float("nan"))
        before = last()[7]
        _lib.check(L.chore_conv2d_bwd_weight(h, dt, taps, x.data_ptr(), B, H, W, cin, None if st is None else st.data_ptr(),
                                             None if gamma is None else gamma.data_ptr(), None if beta is None else beta.data_ptr(),
                                             dy.data_ptr(), cout, dw, db, ws.data_ptr(), None if amax is None else amax.data_ptr(),
                                             stream), h, "bwd_weight %s %s" % (cid, mode))
        torch.cuda.synchronize()
        rec = last()
        assert rec[7] == before + 1, (cid, mode, "one weight-gradient launch per call", before, rec[7])
        key = cid + "|" + mode
        out[key + "|dw"] = dwbuf.cpu().numpy()
        if dbbuf is not None:
            out[key + "|db"] = dbbuf.cpu().numpy()
        out[key + "|page"] = ws[nws:].cpu().numpy()
        out[key + "|rec"] = rec
    np.savez(out_path, **out)


def run_child(tmp_path, tag, env, jobs):
    arrays = {}
    for case, _ in jobs:
        for k, v in inputs_of(case).items():
            arrays[case["id"] + "/" + k] = v
    return RUNNER.run(tmp_path, tag, env, arrays, [(c["id"], m) for c, m in jobs], CHILD_TIMEOUT)


# ------------------------------------------------------------------------------------------------ the checks
def _bits(a):
    """float32 bit patterns, a zero's sign dropped"""
    return (np.asarray(a, dtype=np.float32) + np.float32(0.0)).view(np.uint32)


def where_text(case, rec, idx):
    o, c, t = (int(v) for v in idx)
    ct = int(rec[3])
    tap = "tap (%d, %d)" % (t // 3, t % 3) if case["taps"] == 9 else "tap 0"
    return "o %d (%d of its %d-channel tile) c %d (%d of its %d-channel tile) %s; witness %s" % (o, o % ct, ct, c, c % ct, ct, tap,
                                                                                                [int(v) for v in rec])


def unguard(buf, n, margin, what, fails):
    if not (np.array_equal(buf[:margin], np.full(margin, SENTINEL, np.float32)) and
            np.array_equal(buf[margin + n:], np.full(margin, SENTINEL, np.float32))):
        fails.append("wrote outside %s (%d margin elements changed)" % (what, int((buf[:margin] != SENTINEL).sum() + (buf[margin + n:] != SENTINEL).sum())))
    return buf[margin:margin + n]


def check_job(case, mode, res, worst):
    """-> (list of failure texts, coverage key)"""
    key = case["id"] + "|" + mode
    cin, cout, taps = case["cin"], case["cout"], case["taps"]
    rec = res[key + "|rec"]
    wkey = wc.witness_key(rec)
    fails = []
    # the witness agrees with what was asked for
    flags = int(rec[6])
    if int(rec[2]) != taps or bool(flags & wc.FLAG_GN) != (case["kind"] != "exact") or bool(flags & wc.FLAG_DBIAS) != case["bias"]:
        fails.append("the witness does not describe this call: %s" % [int(v) for v in rec])
    if not 1 <= int(rec[4]) <= max(1, int(rec[5])):
        fails.append("S = %d shares of %d tiles" % (int(rec[4]), int(rec[5])))
    # d. guards
    dw = unguard(res[key + "|dw"], cout * cin * taps, DW_MARGIN, "dW", fails).reshape(cout, cin, taps)
    got = [("dW", dw)]
    if case["bias"]:
        got.append(("dbias", unguard(res[key + "|db"], cout, DB_MARGIN, "dbias", fails)))
    if not np.array_equal(res[key + "|page"], np.full(WS_PAGE, WS_BYTE, np.uint8)):
        fails.append("wrote behind its workspace (%d bytes of the sentinel page changed)" % int((res[key + "|page"] != WS_BYTE).sum()))
    ref = reference(case, mode)
    text = []
    for i, (what, g) in enumerate(got):
        bad = ~np.isfinite(g)
        if bad.any():
            first = np.argwhere(bad)[0]
            fails.append("%d entries of %s not written or not finite, first at %s" %
                         (int(bad.sum()), what, where_text(case, rec, first) if what == "dW" else "channel %d" % first[0]))
            continue
        if case["kind"] == "zero":
            # c. zero gradient
            if g.any():
                fails.append("%s is not 0 for dy == 0: %d entries, largest %.3e" % (what, int((g != 0).sum()), float(np.abs(g).max())))
            text.append("%s == 0" % what)
            continue
        r = ref[i].reshape(g.shape)
        if case["kind"] == "exact":
            # b. exact
            ne = _bits(g) != _bits(r.astype(np.float32))
            if ne.any():
                first = np.argwhere(ne)[0]
                fails.append("%d of %d entries of %s differ from the exact result, first at %s: %r instead of %r" %
                             (int(ne.sum()), g.size, what, where_text(case, rec, first) if what == "dW" else "channel %d" % first[0],
                              float(g[tuple(first)]), float(r[tuple(first)])))
            text.append("%s exact (largest %d)" % (what, int(np.abs(r).max())))
            continue
        # a. values
        bmax, bl2 = BOUNDS[mode]
        g64 = g.astype(np.float64)
        emax, el2 = conv_ref.rel_max(g64, r), conv_ref.rel_l2(g64, r)
        w = worst.setdefault(mode, [0.0, 0.0])
        w[0], w[1] = max(w[0], emax), max(w[1], el2)
        if not emax <= bmax:
            first = np.unravel_index(np.abs(g64 - r).argmax(), g.shape)
            fails.append("%s: max error %.3e of the largest entry, bound %.3e, at %s" %
                         (what, emax, bmax, where_text(case, rec, first) if what == "dW" else "channel %d" % first[0]))
        if bl2 is not None and not el2 <= bl2:
            fails.append("%s: relative L2 error %.3e, bound %.3e" % (what, el2, bl2))
        text.append("%s max %.2e (bound %.0e) L2 %.2e" % (what, emax, bmax, el2))
    print("  %-16s %-4s %-32s S %3d tiles %4d  %s%s" % (case["id"], mode, wkey, int(rec[4]), int(rec[5]), "; ".join(text), "  FAILED" if fails else ""))
    return ["%s %s %s: %s" % (case["id"], mode, wkey, f) for f in fails], wkey


_RESULTS = {}      # switch set -> (failures, coverage keys seen), or the text of why its child gave no result


def run_set(name, tmp_path):
    """the checked results of a switch set.  Its child runs once per session whatever becomes of it: a set whose child failed is
    recorded as such and fails every test that asks for it again, without a second start"""
    if name not in _RESULTS:
        jobs = wc.jobs_of(name)
        print("switch set %s %s: %d launches" % (name, wc.SWITCH_SETS[name][0], len(jobs)))
        _RESULTS[name] = "the child of switch set %s did not finish" % name
        try:
            res, path = run_child(tmp_path, name, wc.SWITCH_SETS[name][0], jobs)
        except BaseException as ex:      # (pytest.fail's exception derives from BaseException)
            _RESULTS[name] = "switch set %s gave no result: %s" % (name, str(ex)[:2000])
            raise
        fails, seen, worst = [], set(), {}
        try:
            for case, mode in jobs:
                f, wkey = check_job(case, mode, res, worst)
                fails += f
                seen.add(wkey)
        finally:
            res.close()
            os.remove(path)
        print("switch set %s: worst [max, L2] per mode %s" % (name, json.dumps(worst, default=float)))
        _RESULTS[name] = (fails, seen)
    if isinstance(_RESULTS[name], str):
        pytest.fail(_RESULTS[name], pytrace=False)
    return _RESULTS[name]


@pytest.mark.parametrize("name", list(wc.SWITCH_SETS))
def test_switch_set(tmp_path, name):
    fails, seen = run_set(name, tmp_path)
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails[:40])
    assert len(seen) >= 1


def test_no_uninitialised_lds_read(tmp_path):
    """one case per kernel in every mode, default switches: the results with every CU's LDS poisoned after every launch equal the
    unpoisoned ones bit for bit"""
    jobs = [(c, m) for c, m in wc.jobs_of("default") if c["poison"] and c["kind"] != "zero"]
    kernels = set()
    a, pa = run_child(tmp_path, "clean", {}, jobs)
    try:
        b, pb = run_child(tmp_path, "poison", wc.POISON_ENV, jobs)
    except BaseException:
        a.close()
        os.remove(pa)
        raise
    try:
        fails = []
        for c, m in jobs:
            k = c["id"] + "|" + m
            kernels.add(wc.witness_key(a[k + "|rec"])[0])
            assert np.array_equal(a[k + "|rec"][:7], b[k + "|rec"][:7])
            for part in ("|dw", "|db"):
                if k + part in a.files and not np.array_equal(a[k + part].view(np.uint32), b[k + part].view(np.uint32)):
                    fails.append("%s %s %s%s" % (c["id"], m, wc.witness_key(a[k + "|rec"]), part))
        assert not fails, fails
        assert kernels == set(wc.KERNELS.values()), kernels
    finally:
        for r, p in ((a, pa), (b, pb)):
            r.close()
            os.remove(p)


def test_every_shipped_instantiation_was_reached(tmp_path):
    """wgrad_cases.COVERAGE against what chore_debug_last_wgrad reported over all switch sets"""
    seen, lost = set(), []
    for name in wc.SWITCH_SETS:
        if isinstance(_RESULTS.get(name), str):      # its child failed in test_switch_set: not started a second time
            lost.append(_RESULTS[name])
        else:
            seen |= run_set(name, tmp_path)[1]
    unknown = sorted(k for k in seen if k not in wc.COVERAGE)
    missing = sorted(k for k, why in wc.COVERAGE.items() if why is None and k not in seen)
    print("coverage table (%d rows, %d to reach, %d reached by the matrix):" % (len(wc.COVERAGE), sum(w is None for w in wc.COVERAGE.values()),
                                                                             len(seen & set(wc.COVERAGE))))
    for k, why in wc.COVERAGE.items():
        print("  %-36s %s" % (k, "reached" if k in seen else ("NOT REACHED" if why is None else "not covered: " + why)))
    assert not lost, "\n".join(["%d switch sets gave no result, the table cannot be checked" % len(lost)] + lost)
    assert not unknown, ("the witness reported instantiations the table does not name", unknown)
    assert not missing, ("no case reached", missing)
    # ... and under DEFAULT switches the kernel of the largest layers of the step
    assert ("w64x3pc", "x3", 9, "xcd") in run_set("default", tmp_path)[1]


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "--child":
    sys.path.insert(0, REPO)
    child_main(*sys.argv[2:5])
