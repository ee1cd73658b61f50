"""GPU: every convolution kernel family (conv_lds / conv_small / conv_pc / conv_mw / conv_rw _kernel) at every tiling its launcher
can pick, against the float64 reference of tests/conv_ref.py.

Cases (tests/conv_cases.py) go through chore_conv2d_fwd / chore_conv2d_bwd_data.  The library reads its switches once per
process, so every switch set runs in a child process of its own (this file with --child); the parent makes the inputs on the
CPU with fixed seeds and hands them over in an .npz, so device and reference see the same bits, and a layer's reference is
computed once and reused across the switch sets.  A child returns, per case and mode, the output buffer, the statistics cells
of the output, the chore_debug_last_conv record (which kernel and tiling the launch chose) and what chore_conv_plan says of the
same arguments in that process: the two must agree for every job.

Checks per case
  a. values, random input through GroupNorm ("gn"): fp32 and fp16 x 3 within 2e-5 of the reference's largest entry; bf16 within
     3e-2 of it and 1.5e-2 relative L2, the reference fed the bf16-rounded input (the bounds of test_gpu_train_ops.py).  fp16
     (half tensors) has no per-layer bound in the project; its bound comes from the reference alone: the error of the storage
     rounding model (conv_ref.storage_model: normalised activation and output rounded to half) against float64 on the same
     half input, times 4 for the maximum and times 2 for the relative L2 (the kernel also splits the weights and accumulates in
     fp32, and a maximum over millions of roundings fluctuates more than their norm).  Those bounds must stay below the
     encoder-level fp16 bounds (2e-2 / 4e-3, test_gpu_encoder.py).
  b. exact cases ("plain" forward and "bwd" data gradient, no GroupNorm): inputs and weights in {-1, 0, 1}, the reference's
     largest |y| asserted <= 256 (exact in bf16; fp16 holds 2048): equal to the reference bit for bit in every mode.  A wrong
     tap, flip, halo row or channel chunk at a tile edge shows here; a mismatch is reported with its position in the tile.
  c. the output lives inside a larger buffer: the payload is pre-filled with NaN and must come back finite, the margins (one
     image row of output on each side) hold a sentinel and must come back unchanged.
  d. output statistics: the decoded cells against float64 sums of the stored output, 2e-6 relative (test_gpu_conv_mw.py).
  e. one more pair of children on one case per family, without and with CHORE_LDS_POISON (every CU's LDS filled with quiet
     NaNs after every launch): bit-identical outputs; a kernel that reads LDS nobody wrote fails.
  f. coverage: every row of conv_cases.COVERAGE that is marked covered was reported by the witness for at least one case.

Measured on an MI355X (worst over the matrix, next to the bound):
  mode    worst max error (bound)      worst relative L2 (bound)    where
    fp32    1.6e-06 (2e-5)               6.1e-07                      default switches
    fp16x3  1.7e-06 (2e-5)               5.4e-07                      CHORE_CONV_MW_FILL=256 CHORE_CONV_MW_TH2=1
    bf16    4.5e-03 (3e-2)               2.9e-03 (1.5e-2)             every bf16 switch set
    fp16    5.3e-04 (4 x model, 2.1e-3)  2.98e-04 (2 x model, 6.0e-4) default switches; 0.26 and 0.50 of the bounds at worst
    statistics of the output: 1.9e-07 relative at worst (2e-6); the exact cases, the guard margins, the poisoned-LDS run and the
    coverage table (122 rows, 86 to reach, 86 reached) held in all 11 switch sets, 688 launches.
  fp16 storage rounding model per case, max / relative L2 of the reference's largest entry (the kernels' measured errors equal
  the model's to the digits shown in all but the first case, 3.66e-04: the kernels are as exact as the number format allows):
    p256_128  3.57e-04 / 2.93e-04   p128_64   3.64e-04 / 2.98e-04   p64_32    4.10e-04 / 2.92e-04   m64_64    3.70e-04 / 2.94e-04
    m64_64r   4.07e-04 / 3.01e-04   m256_128  4.43e-04 / 2.93e-04   m128_128  4.21e-04 / 2.98e-04   s256_128  3.35e-04 / 2.93e-04
    s128_64   3.62e-04 / 2.82e-04   s64_64    3.99e-04 / 2.87e-04   sr128_32  4.25e-04 / 2.99e-04   sr256_64  3.89e-04 / 3.00e-04
    r32_128   4.03e-04 / 2.93e-04   r32_64    3.87e-04 / 2.91e-04   r32_32    3.85e-04 / 2.83e-04   t128_64   4.26e-04 / 2.93e-04
    t64_32    3.99e-04 / 2.91e-04   h64_128   3.69e-04 / 2.92e-04   d4x128    3.71e-04 / 2.93e-04   d2x128    3.97e-04 / 2.94e-04
    d2x64     4.33e-04 / 2.93e-04   d4x64     3.88e-04 / 2.91e-04   w256_256  4.50e-04 / 2.91e-04   w128_256  4.11e-04 / 2.92e-04
    w128_256p 4.55e-04 / 2.92e-04   w64_128   5.00e-04 / 2.92e-04   w64_128r  4.16e-04 / 2.94e-04   o128_128  4.05e-04 / 2.97e-04
    o64_64    3.85e-04 / 2.95e-04   o64_64r   4.47e-04 / 2.90e-04
"""
import ctypes
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as cc      # noqa: E402
import conv_plan_cases as pcs  # noqa: E402
import conv_ref              # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 7.0
TORCH_DT = {"fp32": torch.float32, "x3": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
EXACT_MAX = 256          # the largest |y| an exact case may have: integers up to 256 are exact in bf16
BOUNDS = {"fp32": (2e-5, None), "x3": (2e-5, None), "bf16": (3e-2, 1.5e-2)}      # (max, relative L2) of the reference's largest entry
FP16_ENCODER_BOUNDS = (2e-2, 4e-3)
STAT_TOL = 2e-6


# ------------------------------------------------------------------------------------------------ inputs and references
def make_inputs(case):
    """the tensors of a case as numpy arrays (NHWC activations, (O, C, kh, kw) weights); fixed seed per case"""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    B, H, W, cin, cout = (case[k] for k in ("B", "H", "W", "cin", "cout"))
    k = 3 if case["taps"] == 9 else 1
    d = {}
    if case["kind"] == "gn":
        d["x"] = (rng.standard_normal((B, H, W, cin), dtype=np.float32) * 1.5 + 0.3).astype(np.float32)
        d["w"] = (rng.standard_normal((cout, cin, k, k), dtype=np.float32) / np.sqrt(cin * k * k)).astype(np.float32)
        d["gamma"] = (rng.random(cin, dtype=np.float32) + 0.5).astype(np.float32)
        d["beta"] = (rng.standard_normal(cin, dtype=np.float32) * 0.2).astype(np.float32)
        if case["bias"]:
            d["bias"] = (rng.standard_normal(cout, dtype=np.float32) * 0.1).astype(np.float32)
    else:
        d["x"] = rng.integers(-1, 2, (B, H, W, cin), dtype=np.int8)
        # "bwd": the LAYER's weight, (layer Cout = cin of the launched convolution, layer Cin = cout)
        d["w"] = rng.integers(-1, 2, (cout, cin, k, k) if case["kind"] == "plain" else (cin, cout, k, k), dtype=np.int8)
        if case["bias"] and case["kind"] == "plain":
            d["bias"] = rng.integers(-1, 2, cout, dtype=np.int8)
    return d


_INPUTS, _REFS, _MODEL = {}, {}, {}


def inputs_of(case):
    if case["id"] not in _INPUTS:
        _INPUTS[case["id"]] = make_inputs(case)
    return _INPUTS[case["id"]]


def _storage(mode):
    return "fp32" if mode == "x3" else mode


def reference(case, mode):
    """float64 reference of a case as the mode's storage sees the input; computed once per (layer, storage type)"""
    exact = case["kind"] != "gn"
    key = (case["id"], "exact" if exact else _storage(mode))
    if key not in _REFS:
        d = inputs_of(case)
        f32 = {k: np.asarray(v, dtype=np.float32) for k, v in d.items()}
        xs = conv_ref.as_stored(f32["x"], "fp32" if exact else mode)
        if case["kind"] == "bwd":
            _REFS[key] = conv_ref.data_gradient(xs, f32["w"])
        else:
            _REFS[key] = conv_ref.forward(xs, f32["w"], f32.get("bias"), f32.get("gamma"), f32.get("beta"))
        if exact:
            top = np.abs(_REFS[key]).max()
            assert 0 < top <= EXACT_MAX, (case["id"], top)
            assert np.array_equal(_REFS[key], np.rint(_REFS[key]))
    return _REFS[key]


def fp16_bounds(case):
    """(max bound, L2 bound, model max, model L2) of a "gn" case in the fp16 mode, from the reference alone"""
    if case["id"] not in _MODEL:
        d = inputs_of(case)
        xs = conv_ref.as_stored(d["x"], "fp16")
        model = conv_ref.storage_model(xs, d["w"], d.get("bias"), d["gamma"], d["beta"], "fp16")
        ref = reference(case, "fp16")
        m, l2 = conv_ref.rel_max(model, ref), conv_ref.rel_l2(model, ref)
        assert 4 * m < FP16_ENCODER_BOUNDS[0] and 2 * l2 < FP16_ENCODER_BOUNDS[1], (case["id"], m, l2)
        _MODEL[case["id"]] = (4 * m, 2 * l2, m, l2)
    return _MODEL[case["id"]]


# ------------------------------------------------------------------------------------------------ the child process
def child_main(in_path, job_path, out_path):
    from chore_amd import _lib
    jobs = json.load(open(job_path))
    data = np.load(in_path)
    dev = torch.device("cuda", 0)
    h = _lib.handle(0)
    L = _lib.lib
    stream = torch.cuda.current_stream().cuda_stream
    code = {"fp32": _lib.F32, "bf16": _lib.BF16, "x3": _lib.F16X3, "fp16": _lib.F16}
    cases = {c["id"]: c for c in cc.cases()}
    out = {}

    def ptr(t):
        return None if t is None else t.data_ptr()

    def last():
        rec = (ctypes.c_int * 8)()
        assert L.chore_debug_last_conv(h, rec, 8) == 8
        return np.array(list(rec), np.int64)

    for cid, mode in jobs:
        c = cases[cid]
        B, H, W, cin, cout, taps = (c[k] for k in ("B", "H", "W", "cin", "cout", "taps"))
        dt, tdt = code[mode], TORCH_DT[mode]

        def get(name, t=torch.float32):
            key = cid + "/" + name
            return torch.from_numpy(data[key].astype(np.float32)).to(t).to(dev).contiguous() if key in data.files else None
        x, w, bias, gamma, beta = get("x", tdt), get("w"), get("bias"), get("gamma"), get("beta")
        n, margin = B * H * W * cout, W * cout
        buf = torch.full((n + 2 * margin,), SENTINEL, dtype=tdt, device=dev)
        buf[margin:margin + n] = float("nan")
        y = buf.data_ptr() + margin * buf.element_size()
        ws = torch.empty(max(16, L.chore_conv2d_workspace_bytes(dt, taps, cin, cout)), dtype=torch.uint8, device=dev)
        assert L.chore_conv2d_workspace_bytes(dt, taps, cin, cout) > 0, (cid, mode)
        sty = torch.zeros(L.chore_gn_stats_bytes(B), dtype=torch.uint8, device=dev)
        before = last()[7]
        if c["kind"] == "bwd":
            amax = None
            if mode == "x3":
                amax = torch.zeros(L.chore_amax_bytes(), dtype=torch.uint8, device=dev)
                _lib.check(L.chore_absmax_f32(h, x.data_ptr(), x.numel(), amax.data_ptr(), stream), h, "absmax")
            _lib.check(L.chore_conv2d_bwd_data(h, dt, taps, x.data_ptr(), B, H, W, cin, w.data_ptr(), cout, y, ws.data_ptr(), ptr(amax),
                                               stream), h, "bwd_data %s %s" % (cid, mode))
        else:
            st = None
            if gamma is not None:
                st = torch.zeros(L.chore_gn_stats_bytes(B), dtype=torch.uint8, device=dev)
                _lib.check(L.chore_gn_stats(h, dt, x.data_ptr(), B, H * W, cin, st.data_ptr(), 1, stream), h, "gn_stats")
            _lib.check(L.chore_conv2d_fwd(h, dt, taps, x.data_ptr(), B, H, W, cin, ptr(st), ptr(gamma), ptr(beta), w.data_ptr(), ptr(bias),
                                          cout, y, sty.data_ptr(), ws.data_ptr(), stream), h, "fwd %s %s" % (cid, mode))
        torch.cuda.synchronize()
        rec = last()
        assert rec[7] == before + 1, (cid, mode, "one convolution launch per call", before, rec[7])
        key = cid + "|" + mode
        out[key + "|y"] = (buf if tdt == torch.float32 else buf.view(torch.int16)).cpu().numpy()
        out[key + "|rec"] = rec
        plan = (ctypes.c_int * 8)()
        assert L.chore_conv_plan(*pcs.plan_args(c, mode), plan, 8) == 7, (cid, mode)
        out[key + "|plan"] = np.array(list(plan)[:7], np.int64)
        if c["kind"] != "bwd":
            out[key + "|st"] = sty.cpu().numpy().view(np.int64)
    np.savez(out_path, **out)


_DEAD = ""         # why no further child may start: set once a child was killed by a signal, aborted or ran into its time limit


def run_child(tmp_path, tag, env, jobs):
    """one subprocess for one set of switches -> its .npz (lazily loaded)"""
    global _DEAD
    in_path, job_path, out_path = (str(tmp_path / ("%s_%s" % (tag, s))) for s in ("in.npz", "jobs.json", "out.npz"))
    arrays = {}
    for case, _ in jobs:
        for k, v in inputs_of(case).items():
            arrays[case["id"] + "/" + k] = v
    np.savez(in_path, **arrays)
    json.dump([(c["id"], m) for c, m in jobs], open(job_path, "w"))
    e = dict(os.environ)
    for k in list(e):
        if k.startswith("CHORE_CONV") or k in ("CHORE_NO_CONV_SMALL", "CHORE_PC_FORCE", "CHORE_LDS_POISON"):
            del e[k]
    e.update(env)
    if _DEAD:
        pytest.fail("not started: an earlier child of this module died abnormally (%s); nothing more runs on that GPU" % _DEAD, pytrace=False)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", in_path, job_path, out_path], env=e, capture_output=True,
                           text=True, timeout=900)
    except subprocess.TimeoutExpired as ex:
        _DEAD = "switch set %s: no end after %d s" % (tag, ex.timeout)
        pytest.fail(_DEAD, pytrace=False)
    finally:
        os.remove(in_path)
    if r.returncode != 0:
        # 1: a Python exception, the process itself ended in order.  Anything else (a signal, an abort, a GPU fault) bars every
        # later child of this module: a card that has just faulted gets no further work from here
        if r.returncode != 1:
            _DEAD = "switch set %s: exit status %d" % (tag, r.returncode)
        pytest.fail("child of switch set %s ended with status %d:\n%s" % (tag, r.returncode, r.stderr[-3000:]), pytrace=False)
    return np.load(out_path), out_path


# ------------------------------------------------------------------------------------------------ the checks
def as_float64(raw, mode):
    if TORCH_DT[mode] == torch.float32:
        return raw.astype(np.float64)
    return torch.from_numpy(raw).view(TORCH_DT[mode]).double().numpy()


def where_text(rec, idx):
    """a position in the output, and in the tile of the launch the witness record `rec` describes: rec[1] rows (conv_rw has no row
    tile: its workgroups walk the pixels linearly) x 32 pixels x rec[2] channels"""
    b, yy, xx, ch = (int(v) for v in idx)
    rows, nt = int(rec[1]), int(rec[2])
    row = "row %d (%d of its %d-row tile)" % (yy, yy % rows, rows) if rows else "row %d" % yy
    return "image %d %s column %d (%d of its 32-pixel tile) channel %d (%d of its %d-channel tile)" % (b, row, xx, xx % 32, ch, ch % nt, nt)


def check_job(case, mode, res, worst):
    """-> (list of failure texts, coverage key)"""
    key = case["id"] + "|" + mode
    B, H, W, cout = (case[k] for k in ("B", "H", "W", "cout"))
    n, margin = B * H * W * cout, W * cout
    raw = res[key + "|y"]
    rec = res[key + "|rec"]
    wkey = cc.witness_key(case, mode, rec)
    fails = []
    # the launch is the plan's (chore_conv_plan in the child, under its switches): family, tiling and flags, and the class that names them
    plan = res[key + "|plan"]
    if not (np.array_equal(rec[:6], plan[:6]) and int(rec[6]) == case["cin"] and pcs.CLASS_NAMES[int(plan[6])] == pcs.class_name(case, rec)):
        fails.append("launched %r, chore_conv_plan says %r" % (list(rec[:7]), list(plan)))
    buf = as_float64(raw, mode)
    # c. every output written, nothing else
    if not (np.array_equal(buf[:margin], np.full(margin, SENTINEL)) and np.array_equal(buf[margin + n:], np.full(margin, SENTINEL))):
        fails.append("wrote outside its output (%d margin elements changed)" % int((buf[:margin] != SENTINEL).sum() + (buf[margin + n:] != SENTINEL).sum()))
    y = buf[margin:margin + n].reshape(B, H, W, cout)
    bad = ~np.isfinite(y)
    if bad.any():
        fails.append("%d outputs not written or not finite, first at %s" % (int(bad.sum()), where_text(rec, np.argwhere(bad)[0])))
        return ["%s %s %s: %s" % (case["id"], mode, wkey, f) for f in fails], wkey
    ref = reference(case, mode)
    text = ""
    if case["kind"] == "gn":
        # a. values
        if mode == "fp16":
            bmax, bl2, mmax, ml2 = fp16_bounds(case)
            text = " (model %.2e / %.2e)" % (mmax, ml2)
        else:
            bmax, bl2 = BOUNDS[mode]
        emax = conv_ref.rel_max(y, ref)
        el2 = conv_ref.rel_l2(y, ref)
        w = worst.setdefault(mode, [0.0, 0.0, 0.0, 0.0])
        w[0], w[1] = max(w[0], emax), max(w[1], el2)
        w[2], w[3] = max(w[2], emax / bmax), max(w[3], el2 / bl2 if bl2 else 0.0)
        if not emax <= bmax:
            idx = np.unravel_index(np.abs(y - ref).argmax(), y.shape)
            fails.append("max error %.3e of the largest entry, bound %.3e, at %s" % (emax, bmax, where_text(rec, idx)))
        if bl2 is not None and not el2 <= bl2:
            fails.append("relative L2 error %.3e, bound %.3e" % (el2, bl2))
        text = "max %.2e (bound %.2e) L2 %.2e%s" % (emax, bmax, el2, text)
    else:
        # b. exact
        want = torch.from_numpy(ref).to(TORCH_DT[mode])
        want = want.numpy() if TORCH_DT[mode] == torch.float32 else want.view(torch.int16).numpy()
        got = raw[margin:margin + n].reshape(B, H, W, cout)
        ne = want.view(np.uint32 if want.dtype == np.float32 else np.int16) != got.view(np.uint32 if got.dtype == np.float32 else np.int16)
        if ne.any():
            idx = np.argwhere(ne)[0]
            fails.append("%d of %d outputs differ from the exact result, first at %s: %r instead of %r" %
                         (int(ne.sum()), n, where_text(rec, idx), float(y[tuple(idx)]), float(ref[tuple(idx)])))
        text = "exact, largest |y| %d" % int(np.abs(ref).max())
    # d. statistics of the stored output
    if case["kind"] != "bwd":
        got_s, want_s = conv_ref.stat_values(res[key + "|st"]), conv_ref.group_sums(y)
        es = np.abs(got_s - want_s).max() / np.abs(want_s).max()
        worst["stats"] = max(worst.get("stats", 0.0), es)
        if not es <= STAT_TOL:
            fails.append("output statistics off by %.3e relative, bound %.0e" % (es, STAT_TOL))
        text += " stats %.1e" % es
    print("  %-16s %-4s %-44s %s%s" % (case["id"], mode, wkey, text, "  FAILED" if fails else ""))
    return ["%s %s %s: %s" % (case["id"], mode, wkey, f) for f in fails], wkey


_RESULTS = {}      # switch set -> (failures, coverage keys seen), or the text of why its child gave no result


def run_set(name, tmp_path):
    """the checked results of a switch set.  Its child runs once per session whatever becomes of it: a set whose child failed is
    recorded as such and fails every test that asks for it again, without a second start"""
    if name not in _RESULTS:
        jobs = cc.jobs_of(name)
        print("switch set %s %s: %d launches" % (name, cc.SWITCH_SETS[name][0], len(jobs)))
        _RESULTS[name] = "the child of switch set %s did not finish" % name
        try:
            res, path = run_child(tmp_path, name, cc.SWITCH_SETS[name][0], jobs)
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
        print("switch set %s: worst [max, L2, max / bound, L2 / bound] per mode %s" % (name, json.dumps(worst, default=float)))
        _RESULTS[name] = (fails, seen)
    if isinstance(_RESULTS[name], str):
        pytest.fail(_RESULTS[name], pytrace=False)
    return _RESULTS[name]


@pytest.mark.parametrize("name", list(cc.SWITCH_SETS))
def test_switch_set(tmp_path, name):
    fails, seen = run_set(name, tmp_path)
    assert not fails, "\n".join(["%d failures" % len(fails)] + fails[:40])
    assert len(seen) >= 1


def test_no_uninitialised_lds_read(tmp_path):
    """one case per family in every mode, default switches: the outputs with every CU's LDS poisoned after every launch equal the
    unpoisoned ones bit for bit"""
    jobs = [(c, m) for c, m in cc.jobs_of("default") if c["poison"]]
    fams = set()
    a, pa = run_child(tmp_path, "clean", {}, jobs)
    b, pb = run_child(tmp_path, "poison", cc.POISON_ENV, jobs)
    try:
        fails = []
        for c, m in jobs:
            k = c["id"] + "|" + m
            fams.add(cc.witness_key(c, m, a[k + "|rec"])[0])
            assert np.array_equal(a[k + "|rec"][:7], b[k + "|rec"][:7])
            for part in ("|y", "|st"):
                if k + part in a.files and not np.array_equal(a[k + part], b[k + part]):
                    fails.append("%s %s %s%s" % (c["id"], m, cc.witness_key(c, m, a[k + "|rec"]), part))
        assert not fails, fails
        assert fams == {"lds", "small", "pc", "mw", "rw"}, fams
    finally:
        for r, p in ((a, pa), (b, pb)):
            r.close()
            os.remove(p)


def test_every_shipped_instantiation_was_reached(tmp_path):
    """conv_cases.COVERAGE against what chore_debug_last_conv reported over all switch sets"""
    seen, lost = set(), []
    for name in cc.SWITCH_SETS:
        if isinstance(_RESULTS.get(name), str):      # its child failed in test_switch_set: not started a second time
            lost.append(_RESULTS[name])
        else:
            seen |= run_set(name, tmp_path)[1]
    unknown = sorted(k for k in seen if k not in cc.COVERAGE)
    missing = sorted(k for k, why in cc.COVERAGE.items() if why is None and k not in seen)
    print("coverage table (%d rows, %d to reach, %d reached by the matrix):" % (len(cc.COVERAGE), sum(w is None for w in cc.COVERAGE.values()),
                                                                             len(seen & set(cc.COVERAGE))))
    for k, why in cc.COVERAGE.items():
        print("  %-44s %s" % (k, "reached" if k in seen else ("NOT REACHED" if why is None else "not covered: " + why)))
    assert not lost, "\n".join(["%d switch sets gave no result, the table cannot be checked" % len(lost)] + lost)
    assert not unknown, ("the witness reported instantiations the table does not name", unknown)
    assert not missing, ("no case reached", missing)


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "--child":
    sys.path.insert(0, REPO)
    child_main(*sys.argv[2:5])
