"""CPU: what tests/test_gpu_query_kernels.py covers, checked without a GPU.
  * every kernel name the expectations of query_plan_cases.py hold, under every switch set, has a case in query_kernel_cases.py;
    the rows that file adds to the plan file's agree with chore_query_plan;
  * every instantiation launch_query_fwd and launch_query_bwd spell out (csrc/query_fwd.hip, csrc/query_bwd.hip) is reached by a
    case or has a row with a reason; the table is printed with the number of cases per instantiation;
  * every operation of the cases has a check in the GPU file, and that file runs every switch set;
  * per case the exclusions stay under their cap and a point lies outside the image, from query_ref alone; the float32 floors
    recorded in query_kernel_cases.FLOORS are what query_ref gives;
  * query_ref reproduces the reference project's own results (tests/golden/query_full.npz, query_train_grads.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest

import query_kernel_cases as kc
import query_plan_cases as qc
import query_ref as qr
from conftest import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSETS = len(qc.SWITCH_SETS)


def test_every_expected_kernel_has_a_case():
    for k in range(NSETS):
        want = {qc.expected(c, k) for c in qc.CASES}
        have = {(name, sort) for _, name, sort in kc.jobs_of(k)}
        assert want <= have, (qc.SWITCH_SETS[k][0], sorted(want - have))
        ids = [kc.case_id(c) for c in kc.selected(k)]
        assert len(ids) == len(set(ids))
        for c in kc.selected(k):
            assert c[3] != 20000 and c[2] * c[3] <= kc.MAX_POINTS
            assert (c[4], c[5]) == (16, 16) or (c[2] == 1 and qc.expected(c, k)[1] == 1), c      # large maps: the sort cases only
            for n in (1, 63, 65):               # the ragged counts of every operation
                assert any(d[0] == c[0] and d[3] == n for d in kc.selected(k)), (c[0], n)


def test_added_rows_agree_with_the_plan():
    from chore_amd import _lib
    for c in kc.EXTRA:
        for k, (_, bits, _) in enumerate(qc.SWITCH_SETS):
            out = (ctypes.c_int * 9)()
            n = _lib.lib.chore_query_plan(*c[:8], bits, out, 9)
            name, sort = qc.expected(c, k)
            assert n == 9 and list(out) == qc.plan_of_name(name, sort, c[6]), (c, k, list(out))


def _spelled(path, start, pattern):
    src = open(os.path.join(REPO, "chore_amd", "csrc", path)).read()
    body = src[src.index(start):]
    return {re.sub(r"\s+", " ", m) for m in re.findall(pattern, body)}


def test_every_instantiation_is_reached():
    table = kc.instantiations()
    # the table's patterns are the ones the two launchers spell out
    spelled = (_spelled("query_fwd.hip", "static int launch_query_fwd_t", r"query_fwd_\w+_kernel<T[^>]*>") |
               _spelled("query_bwd.hip", "static int launch_query_bwd_t", r"launch_k<T[^>]*>"))
    assert spelled == set(table), (sorted(spelled - set(table)), sorted(set(table) - spelled))
    names = [n for v in table.values() for n in v]
    assert len(names) == len(set(names)) == 56
    count = {n: [0] * NSETS for n in names}
    for k in range(NSETS):
        for _, name, _ in kc.jobs_of(k):
            assert name in count, ("a case names a kernel the launchers do not spell out", name)
            count[name][k] += 1
    print("coverage table: %d instantiations, cases under %s" % (len(names), " / ".join(s[0] for s in qc.SWITCH_SETS)))
    for n in names:
        print("  %-78s %s%s" % (n, " / ".join("%2d" % v for v in count[n]), "" if any(count[n]) else "   not reached: " + kc.NOT_REACHED.get(n, "NO REASON")))
    missing = [n for n in names if not any(count[n]) and not kc.NOT_REACHED.get(n)]
    assert not missing, missing
    assert not [n for n in kc.NOT_REACHED if n not in count or any(count[n])], "a reason for an instantiation that is reached, or unknown"


def test_every_case_family_is_run_by_the_gpu_file():
    import test_gpu_query_kernels as t
    ops = {c[0] for k in range(NSETS) for c in kc.selected(k)}
    assert ops == set(kc.OP_NAMES) and ops <= set(t.CHECKS)
    assert t.SETS == [s[0] for s in qc.SWITCH_SETS]
    marks = [m for m in t.test_switch_set.pytestmark if m.name == "parametrize"]
    assert list(marks[0].args[1]) == list(range(NSETS))
    assert any(m.name == "gpu" for m in (t.pytestmark if isinstance(t.pytestmark, list) else [t.pytestmark]))


@pytest.fixture(scope="module")
def by_forward():
    """the distinct cases of all sets, grouped by the reference forward they share"""
    groups = {}
    for k in range(NSETS):
        for c in kc.selected(k):
            groups.setdefault((kc.map_type(c[1]), c[4], c[5], c[2], c[3]), {})[kc.case_id(c)] = c
    return groups


def test_exclusions_and_points_outside_the_image(by_forward):
    floors_seen = {}
    for key, cases in sorted(by_forward.items()):
        c0 = next(iter(cases.values()))
        need32 = any((cid, q) in kc.FLOORS for cid in cases for q in ("dpoints", "step0", "step1"))
        f, f32 = kc.forwards_of(c0, True) if need32 else (kc.forwards_of(c0), None)
        N = key[4]
        ok_out, ok_grad = kc.exclusions(f)
        if N >= 63:
            assert ok_grad.mean() > 1 - kc.MAX_EXCLUDED and ok_out.mean() > 1 - kc.MAX_EXCLUDED, (key, ok_out.mean(), ok_grad.mean())
            assert (~f["in_img"]).any(1).all() if N >= 333 else (~f["in_img"]).any(), ("no point outside the image", key)
            assert (f["border"][~f["in_img"].reshape(-1)] >= kc.BORDER_MIN).any()
        for cid, c in cases.items():
            if c[0] == qc.SURFACE_STEP and N >= 63:
                for k in (0, 1):
                    thr = kc.surface_thr(f, k)
                    _, clamp = qr.surface_step(f, k, thr)
                    assert (ok_grad & ~(clamp < kc.CLAMP_MIN)).mean() > 1 - kc.MAX_EXCLUDED, (cid, k)
                    below = (f["df"][:, k] <= thr)[f["in_img"]].mean()
                    assert 0.2 < below < 0.8, (cid, k, below)               # both sides of the clamp occur
            if f32 is not None and any(k[0] == cid for k in kc.FLOORS):
                for q, (e, b) in kc.floors_of(c, f, f32).items():
                    floors_seen[cid, q] = (e, b)
    # the recorded floors: needed (above the bound they replace), what query_ref gives (BLAS orders differ a little), four times allowed
    for key, (floor, bound) in kc.FLOORS.items():
        e, b = floors_seen[key]
        print("  floor %-46s %-8s recorded %.2e, now %.2e; bound %.2e instead of %.1e" % (key + (floor, e, bound, b)))
        assert floor > b and abs(bound - 4 * floor) <= 0.01 * bound, key
        assert 0.7 * floor <= e <= 1.3 * floor, (key, e, floor)


def test_reference_reproduces_the_reference_projects_results(spec):
    """query_ref against what the reference itself computed: outputs and dpoints of query_full.npz, the parameter and map gradients of
    query_train_grads.npz, within the bounds the GPU test uses.  The fixture places four points on the image border in float32
    (nx or ny == +-1 exactly); float64 sees them a rounding error outside, so there the fixture's own df == 5.0 mask is taken."""
    from chore_amd.utils import synth
    sd = {k: np.asarray(v) for k, v in synth.synth_state_dict(spec, seed=0).items() if k.split(".")[0] in qr.HEADS}
    g, gg = golden("query_full.npz"), golden("query_train_grads.npz")
    feat, tmpx = g["feat"].transpose(0, 2, 3, 1), g["tmpx"].transpose(0, 2, 3, 1)
    B, N = g["points"].shape[:2]
    f = qr.forward(g["points"], g["crop_center"], feat, tmpx, sd)
    gold_in = (g["df"] != 5.0).all(1)
    on_border = f["border"].reshape(B, N) < kc.BORDER_MIN
    assert np.array_equal(f["in_img"][~on_border], gold_in[~on_border]) and on_border.sum() <= 8
    x32, in32 = qr.features_f32(g["points"], g["crop_center"], feat, tmpx)
    assert np.array_equal(in32, gold_in)                      # the float32 restatement has the fixture's mask, border included
    assert np.abs(x32 - f["X"]).max() <= kc.OUT_BOUND
    f["in_img"] = gold_in
    for k in qr.OUT_NAMES:
        r = g[k].reshape(f[k].shape)
        raw = f["raw"][qr.OUT_NAMES.index(k)].reshape(B, N, -1).transpose(0, 2, 1)
        got = np.where(gold_in[:, None, :], raw, qr.OUT_DIST) if k == "df" else f[k]
        assert np.abs(got - r).max() <= kc.OUT_BOUND * max(1, np.abs(r).max()), k
    grads = [g["w_df"], g["w_parts"], g["w_pca"].reshape(B, 9, N), g["w_centers"]]
    stable = f["margin"] > kc.MARGIN_MIN
    assert stable.mean() > 0.95
    dp = qr.backward(f, grads)["dpoints"].reshape(-1, 3)
    assert np.abs(dp - g["dpoints"].reshape(-1, 3))[stable].max() <= kc.GRAD_BOUND * np.abs(g["dpoints"]).max()
    # the training gradients: the fixture's functional leaves out the points it found on a ReLU kink
    masked = [w * gg["stable"][:, None, :] for w in grads]
    back = qr.backward(f, masked)
    pg = qr.param_grads(f, back, masked)
    checked = 0
    for k in gg.files:
        if k.startswith("g_"):
            r = gg[k].reshape(pg[k[2:]].shape)
            assert np.abs(pg[k[2:]] - r).max() <= kc.GRAD_BOUND * np.abs(r).max(), k
            checked += 1
        elif k.startswith("c_"):
            r = gg[k]
            assert np.abs(pg[k[2:]][:16, :24] - r).max() <= kc.GRAD_BOUND * np.abs(pg[k[2:]]).max(), k
            a = pg[k[2:]]
            got = np.array([a.sum(), np.abs(a).sum(), np.sqrt((a ** 2).sum())])
            assert np.abs(got - gg["s_" + k[2:]]).max() <= kc.GRAD_BOUND * gg["s_" + k[2:]][1], k
            checked += 1
    assert checked == 32
    for nm, s, c0, C in (("dfeat", f["sf"], 0, qr.FEAT_C), ("dtmpx", f["st"], qr.FEAT_C + 3, qr.TMPX_C)):
        r = gg[nm].transpose(0, 2, 3, 1)
        got = qr.scatter_map(s, back["dX"][:, c0:c0 + C].reshape(B, N, C), r.shape[1] * r.shape[2]).reshape(r.shape)
        assert np.abs(got - r).max() <= kc.GRAD_BOUND * np.abs(r).max(), nm
    assert len(sd) == 32
