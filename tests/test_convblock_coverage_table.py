"""CPU: what tests/test_gpu_convblock_kernels.py rests on, held before anyone reaches a GPU -- the entry points it covers, the plan of
every launch of every job (convblock_cases.PLANS against csrc/conv_plan.h through tests/conv_plan_sweep.cpp), which kernels the
production blocks take and that a case takes each of them, the `saved` layout against the pinned sizes, the constants against the
sources, the matrix sizes, and the ReLU-kink procedure on the float64 reference alone."""
import os
import re

import numpy as np
import pytest

import conv_cases as cc
import conv_plan_cases as pc
import conv_ref
import convblock_cases as bc
import convblock_ref as br
import wgrad_cases as wc
import workspace_cases as ws
from conftest import REPO

CSRC = os.path.join(REPO, "chore_amd", "csrc")


def _read(*parts):
    return open(os.path.join(REPO, *parts)).read()


def test_entry_points_are_covered():
    names = sorted(set(re.findall(r"\b(chore_convblock_\w+)\s*\(", _read("include", "chore_hip.h"))))
    assert len(names) == 6 and names == sorted(bc.COVERAGE), names
    lib = _read("chore_amd", "_lib.py")
    for n, how in bc.COVERAGE.items():
        assert '"%s"' % n in lib, n
        assert len(how) > 20, n
    # ... and the GPU module calls each of them through the C API
    gpu = _read("tests", "test_gpu_convblock_kernels.py")
    for n in names:
        assert "L.%s(" % n in gpu, n


def test_matrix_sizes():
    assert len(bc.cases()) == bc.N_CASES == len(bc.CASES)
    assert set(bc.N_JOBS) == set(bc.SWITCH_SETS)
    for name, n in bc.N_JOBS.items():
        assert len(bc.jobs_of(name)) == n, (name, len(bc.jobs_of(name)))
    for c in bc.cases():
        assert c["B"] * c["H"] * c["W"] <= bc.MAX_PIXELS and (c["cin"], c["cout"]) in bc.PAIRS + [(32, 128)]
    # the channel pairs are the blocks the encoder builds
    built = {(int(a), int(b)) for a, b in re.findall(r"ConvBlock\((\d+), (\d+)\)", _read("chore_amd", "model", "hgfilter.py"))}
    assert set(bc.PAIRS) == built and "ConvBlock(feat, feat)" in _read("chore_amd", "model", "hgfilter.py")      # (feat = 256)
    # dy magnitudes and variants
    assert {c["dy_scale"] for c in bc.cases()} == set(bc.DY_SCALES) == {1e-7, 1.0, 3e4}
    assert {c["shape"] for c in bc.cases() if c["variants"]} == {"tiny", "ragged"}
    assert set(bc.VARIANTS) == {"zero", "slice1", "slice2", "slice3", "small3"} and bc.VARIANTS["small3"][1] == 2.0 ** -12
    assert len(bc.REFUSED) == 9 and bc.REFUSED_THEN in bc.CASES
    # the environments of the convolution switch sets are conv_cases' own
    for name in ("fill128", "mw0", "lds", "no_small", "rw0", "lds_bf16", "pc_bf16", "rw_bf16"):
        assert bc.SWITCH_SETS[name][0] == cc.SWITCH_SETS[name][0], name
    assert bc.POISON_ENV == cc.POISON_ENV == wc.POISON_ENV
    assert bc.SWITCH_SETS["x3_pc"][0] == wc.SWITCH_SETS["x3_pc"][0] and bc.SWITCH_SETS["x3_v1"][0] == wc.SWITCH_SETS["x3_v1"][0]
    assert "CHORE_CONVBLOCK_SERIAL" in _read("chore_amd", "csrc", "convblock.hip")


@pytest.mark.parametrize("name", [n for n in bc.SWITCH_SETS if n not in ("serial", "x3_pc", "x3_v1")])
def test_plans_are_the_pinned_ones(name):
    """every launch of every job the set's modes allow, under the set's environment: the plan is the pinned row"""
    env, modes = bc.SWITCH_SETS[name]
    jobs = [(c, m) for c in bc.cases() for m in modes]
    lines = [l for c, m in jobs for l in bc.plan_lines(c, m)]
    got = pc.sweep(env, lines)
    i = 0
    for c, m in jobs:
        want = bc.plan_of(name, c, m)
        assert len(want) == len(bc.launches(c, m)) == (8 if c["cin"] != c["cout"] else 6)
        for (role, *_), row in zip(bc.launches(c, m), want):
            assert tuple(int(v) for v in got[i].split()[:6]) == row, (name, c["id"], m, role, got[i], row)
            i += 1
    assert i == len(got)
    # the sets list only what differs from the default's rows
    if name != "default":
        assert bc.PLANS[name] and all(v != bc.PLANS["default"][k] for k, v in bc.PLANS[name].items())
        assert len(bc.PLANS[name]) == bc.N_JOBS[name]


def _keys(set_name, jobs):
    out = set()
    for c, m in jobs:
        for (role, *_), row in zip(bc.launches(c, m), bc.plan_of(set_name, c, m)):
            out.add((role, bc.FAMILIES[row[0]], m))
    return out


def test_every_production_launch_is_reached():
    prod = set()
    for cin, cout, side in bc.PRODUCTION:
        c = dict(B=bc.PRODUCTION_B, H=side, W=side, cin=cin, cout=cout)
        for m in bc.MODES:
            got = pc.sweep({}, bc.plan_lines(c, m))
            prod |= {(role, bc.FAMILIES[int(l.split()[0])], m) for (role, *_), l in zip(bc.launches(c, m), got)}
    reached = _keys("default", bc.jobs_of("default"))
    assert len(prod) == 42
    for k in sorted(prod):
        if k in reached:
            assert k not in bc.REACH_REASONS, k
            continue
        assert k in bc.REACH_REASONS, ("a production block takes this and no case does", k)
        via, why = bc.REACH_REASONS[k]
        assert len(why) > 40 and k in _keys(via, bc.jobs_of(via)), k
    assert set(bc.REACH_REASONS) <= prod
    # in fp32 every launch is conv_lds_kernel; the other modes reach every family
    assert {f for _, f, m in reached if m == "fp32"} == {"lds"}
    assert {f for _, f, m in reached if m != "fp32"} == {"lds", "small", "pc", "mw", "rw"}
    # the poisoned-LDS pair: one case per family and per weight-gradient kernel
    pj = [(bc.CASES[c], m) for c in bc.POISON_CASES for m in bc.MODES]
    assert {f for _, f, _ in _keys("default", pj)} == {"lds", "small", "pc", "mw", "rw"}
    assert {k for c, m in pj for k, _ in bc.wgrad_rows(c, m)} == {1, 2, 3, 4, 5}


def test_every_weight_gradient_kernel_runs_under_a_strided_dy():
    """wgrad3 (the last slice of dy) and wgradd (the whole of dy beside x) read dy with the row stride Cout"""
    seen = {}
    for c in bc.cases():
        for m in bc.MODES:
            for (role, taps, ci, co), (kern, elem) in zip(bc.wgrads(c), bc.wgrad_rows(c, m)):
                if role == "wgrad3" or (role == "wgradd"):
                    seen.setdefault(bc.WGRAD_NAMES[kern], []).append((c["id"], m, role))
    assert set(seen) == set(wc.KERNELS.values()) == set(bc.WGRAD_NAMES.values()), sorted(seen)
    # the forced kernels change some job's weight gradient
    assert bc.jobs_of("x3_pc") and bc.jobs_of("x3_v1")
    # the restated dispatch reads as the source does
    src = _read("chore_amd", "csrc", "train_bwd.hip")
    assert "Cin % 64 == 0 && Cout % 64 == 0" in src and "(taps == 1 || (Cin >= 128 && Cout >= 128 && (long)H * W >= 128 * 128))" in src
    assert "taps == 1 && Cin % 128 == 0 && Cout % 128 == 0 && ((long)H * W) % W128_PX == 0 && (long)B * H * W >= 8 * W128_PX" in src
    assert int(re.search(r"constexpr int (?:\w+ = \d+, )*W128_PX = (\d+)", src).group(1)) == bc.W128_PX
    # the large shape puts conv1's 3x3 weight gradient on the specialised-wave kernel, the 1x1 layers take the 128-channel one
    big = bc.CASES["large_256_256"]
    assert bc.wgrad_kernel("x3", 9, big["B"], big["H"], big["W"], 256, 128) == (4, 2)
    assert bc.wgrad_kernel("x3", 1, 2, 16, 32, 128, 256) == (5, 2)


def test_reasons_of_the_sibling_tables():
    """no launch of the block reaches a scaled 1x1 256 -> 256 convolution or puts a residual on a data gradient; the rows of the
    sibling tables that named chore_convblock_bwd say what is the case now"""
    for c in bc.cases():
        for m in bc.MODES:
            for role, taps, ci, co, bits in bc.launches(c, m):
                assert not (bits & bc.TRAIT_SCALED and bits & bc.TRAIT_RES)
                assert not (bits & bc.TRAIT_SCALED and taps == 1 and ci == co)
    src = re.sub(r"//[^\n]*", "", _read("chore_amd", "csrc", "convblock.hip"))
    assert len(re.findall(r"\bdgrad\(1,", src)) == 1 and "if (d.down) {\n        if ((rc = dgrad(1," in src
    body = re.search(r"auto dgrad = \[&\].*?\n    \};", src, re.S).group(0)
    assert "a.res" not in body
    why = cc.COVERAGE[("rw", "x3s", 256, 256, "res")]
    assert "chore_convblock_bwd" not in why and "test_convblock_coverage_table" in why
    why = wc.COVERAGE[("any", "any", 0, "strided dy, deferred finish")]
    assert "test_gpu_convblock_kernels" in why


def test_saved_layout_is_the_pinned_one():
    n = 0
    for (dt, B, H, W, cin, cout), nbytes in ws.CONVBLOCK_SAVED.items():
        if nbytes:
            assert bc.saved_layout(bc.MODES[dt], B, H, W, cout)["bytes"] == nbytes, (dt, B, H, W, cin, cout)
            n += 1
    assert n >= 60
    src = _read("chore_amd", "csrc", "convblock.hip")
    assert "// saved (forward -> backward): statistics [x | o1 | o2 | y], then o1, o2" in src
    assert "return {c.raw<char>(d.nb), c.raw<char>(d.nb), c.raw<char>(d.nb), c.take<char>(d.nb)," in src
    assert "size_t chore_convblock_out_stats_offset(int B) { return 3 * act_stats_bytes(B); }" in src
    lay = bc.saved_layout("bf16", 3, 5, 7, 256)
    assert lay["sy"] == 3 * bc.stats_bytes(3) and lay["o1"] % 256 == 0 and lay["o2"] % 256 == 0
    # the gradient arena
    assert "// floats of the parameter-gradient arena: dW1 dW2 dW3 [dWd] then (dgamma, dbeta) of bn1, bn2, bn3 [, bn4]" in src
    for cin, cout in bc.PAIRS + [(32, 128)]:
        c1, c2 = cout // 2, cout // 4
        n = 9 * (cin * c1 + c1 * c2 + c2 * c2) + 2 * (cin + c1 + c2) + ((cin * cout + 2 * cin) if cin != cout else 0)
        assert bc.grad_layout(cin, cout)[1] == n


def test_constants_are_the_sources():
    enc = _read("chore_amd", "csrc", "enc_common.h")
    assert int(re.search(r"constexpr int AMAX_CELLS = (\d+);", enc).group(1)) == bc.AMAX_CELLS
    # the window: the maximum is scaled into [2^13, 2^14), a hi / lo pair keeps its 22 bits above 2^-3
    assert "(max |x| * mul in [2^13, 2^14))" in enc and "only above 2^-3" in enc
    assert bc.AMAX_WINDOW_LOG2 == -3 - 14 and bc.VARIANTS["small3"][1] > 2.0 ** bc.AMAX_WINDOW_LOG2
    assert re.search(r"^KINK = 1e-3$", _read("tests", "test_gpu_bwd_operators.py"), re.M) and bc.KINK == 1e-3
    assert bc.NUDGE_CAP == 0.005 and bc.NUDGE_CAP_REF == 0.0025
    gpu = _read("tests", "test_gpu_convblock_kernels.py")
    assert "At most 0.5 % of a tensor may move" in gpu and "KINK = 1e-3" in gpu
    conv = _read("tests", "test_gpu_conv_kernels.py")
    assert 'BOUNDS = {"fp32": (2e-5, None), "x3": (2e-5, None), "bf16": (3e-2, 1.5e-2)}' in conv and "STAT_TOL = 2e-6" in conv
    assert bc.LAYER_BOUNDS == {"fp32": (2e-5, None), "x3": (2e-5, None), "bf16": (3e-2, 1.5e-2)} and bc.STAT_TOL == 2e-6
    assert "times 4 for the maximum and times 2 for the relative L2" in conv and bc.BF16_MODEL_MARGIN == (4.0, 2.0)
    for s in bc.DY_SCALES:            # inside x3_in_scale's window: biased exponent of the maximum in 14 .. 240
        assert 2.0 ** (14 - 127) < s and 6 * s < 2.0 ** (240 - 127)
    assert "if (e >= 14u && e <= 240u)" in enc
    # the depth table: operators chained between dy and each output, in the order convblock.hip launches them -- a data gradient, a
    # GroupNorm backward and a weight gradient count one each
    src = re.sub(r"//[^\n]*", "", _read("chore_amd", "csrc", "convblock.hip"))
    body = src[src.index("int chore_convblock_bwd("):]
    calls = re.findall(r"rc = (dgrad|gn_relu_bwd_impl|conv2d_bwd_weight_impl)\((?:h, dtype, )?(\d)?", body)
    assert [c[0] for c in calls] == ["dgrad", "gn_relu_bwd_impl", "conv2d_bwd_weight_impl", "conv2d_bwd_weight_impl", "dgrad", "gn_relu_bwd_impl",
                                     "conv2d_bwd_weight_impl", "dgrad", "gn_relu_bwd_impl", "dgrad", "gn_relu_bwd_impl", "conv2d_bwd_weight_impl"]
    d_o2 = 0 + 1 + 1                  # dy -> dgrad3 -> gn3 (+ dy2)
    d_o1 = d_o2 + 1 + 1               # -> dgrad2 -> gn2 (+ dy1)
    d_x = d_o1 + 1 + 1                # -> dgrad1 -> gn1 (+ skip: dy, or dgradd -> gn4 at depth 2)
    want = {"dw3": 1, "dwd": 1, "dg3": d_o2, "db3": d_o2, "dg4": 2, "db4": 2, "dw2": d_o2 + 1, "dg2": d_o1, "db2": d_o1, "dw1": d_o1 + 1,
            "dg1": d_x, "db1": d_x, "dx": d_x}
    assert bc.DEPTH == want
    for cin, cout in bc.PAIRS:
        assert set(bc.grad_layout(cin, cout)[0]) | {"dx"} <= set(bc.DEPTH)
    for v, zero in bc.EXACT_ZERO.items():
        assert v in bc.VARIANTS and set(zero) < set(bc.DEPTH)


def test_refused_rows_are_what_the_source_refuses():
    src = _read("chore_amd", "csrc", "convblock.hip")
    assert "if (Cout % 128 || Cin % 32 || Cin > 256 || Cout > 256) return false;" in src
    # both entry points ask the one predicate before their first launch
    for fn in ("fwd", "bwd"):
        body = src[src.index("int chore_convblock_%s(" % fn):]
        assert 0 < body.index("bad_group_channels(d)") < body.index("launch_pack_conv_multi"), fn
    ok = lambda c: c % 32 == 0 and c // 32 in (1, 2, 4, 8)      # noqa: E731  (conv_plan.h, conv_gn_group_ok)
    assert "return channels % 32 == 0 && gs <= 8 && !(gs & (gs - 1));" in _read("chore_amd", "csrc", "conv_plan.h")
    whats = [r[0] for r in bc.REFUSED]
    assert whats == ["Cin 96", "Cin 224", "Cin 48", "Cin 288", "Cout 64", "Cout 384", "CHORE_F16", "B = 0", "Cin != Cout with NULL wd"]
    for what, dt, B, cin, cout, wd, text in bc.REFUSED:
        dims = dt in (0, 1, 2) and B > 0 and cout % 128 == 0 and cin % 32 == 0 and cin <= 256 and cout <= 256
        legal = dims and ok(cin) and (wd or cin == cout)
        assert not legal, what
        # the size functions keep their pinned values: what make_dims accepts still has a size
        if what in ("Cin 96", "Cin 224"):
            assert dims and not ok(cin)
            assert any(k[4] == cin and v for k, v in ws.CONVBLOCK.items()) and any(k[4] == cin and v for k, v in ws.CONVBLOCK_SAVED.items())


_KINKS = {}


@pytest.mark.parametrize("cid", list(bc.CASES))
def test_kink_nudges_stay_small_on_the_reference(cid):
    """the procedure of the GPU module on the float64 reference's own tensors, fp32 and bf16 storage: x under bn1 / bn4, then the
    reference's o1 under bn2 and o2 under bn3 -- few elements move, in few rounds, and no kink is left"""
    case = bc.CASES[cid]
    x, p, _ = br.make_inputs(case)
    for st in ("fp32", "bf16"):
        xs, moved, rounds = br.nudge(conv_ref.as_stored(x, st), br.x_norms(p), bc.KINK)
        assert moved.mean() <= bc.NUDGE_CAP and rounds <= 3, (cid, st, moved.mean(), rounds)
        assert br.kinks(xs, br.x_norms(p), bc.KINK) == 0
        was, now = conv_ref.as_stored(x, st).double().numpy(), xs.double().numpy()
        assert np.array_equal(now[~moved], was[~moved]) and (now[moved] != was[moved]).all()
        f = br.forward(xs, p, st)
        for name, t, norm in (("o1", f["o1"], (p["g2"], p["b2"])), ("o2", f["o2"], (p["g3"], p["b3"]))):
            stats = br.group_stats(t)            # held, as the operator's statistics cells are
            before = br.pre_activation(t, *norm, stats)
            new, moved, rounds = br.nudge(t, [norm], bc.KINK, stats)
            share = moved.mean()
            print("  %-16s %-4s %s: %.3f %% nudged in %d rounds" % (cid, st, name, 100 * share, rounds))
            assert share <= bc.NUDGE_CAP_REF and rounds <= 1, (cid, st, name, share, rounds)
            after = br.pre_activation(new, *norm, stats)
            assert (np.abs(after) >= bc.KINK).all() and (np.sign(after[moved]) == np.where(before[moved] >= 0, 1, -1)).all()
            if st == "fp32":             # ... and no further than needed (a bf16 step is coarser than the margin)
                assert (np.abs(after[moved]) < 2.01 * bc.KINK).all()


def test_reference_backward_is_autograd():
    """convblock_ref.backward writes the GroupNorm backward out (its statistics are an argument); with the tensors' own statistics
    it must be what torch.autograd gives for the three chained layers and the downsample branch"""
    for cid in ("tiny_32_128", "tiny_64_128", "tiny_256_256"):
        x, p, dy = br.make_inputs(bc.CASES[cid])
        xs = conv_ref.as_stored(x, "fp32")
        f = br.forward(xs, p)
        a = br.backward(xs, f["o1"], f["o2"], conv_ref.as_stored(dy, "fp32"), p)
        b = br.backward_autograd(xs, f["o1"], f["o2"], conv_ref.as_stored(dy, "fp32"), p)
        assert set(a) == set(b)
        for k in a:
            assert conv_ref.rel_max(a[k], b[k]) < 1e-12, (cid, k)
