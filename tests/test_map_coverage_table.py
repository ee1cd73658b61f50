"""CPU: the coverage table of tests/test_gpu_map_kernels.py (map_cases.COVERAGE) names every entry point of the encoder's map
operators in chore_amd/_lib.py, every case family is run by a GPU test, and the constants the shapes were chosen around are the ones
in csrc/enc_misc.hip and csrc/enc_common.h: a renamed entry point, a family without a test or a changed tile size fails here, before
anyone reaches a GPU.  Also here, because they need no GPU: the bicubic matrix of tests/map_ref.py against F.interpolate, the
12-candidate window of up2_bwd_kernel against that matrix, the round trip of the statistics cells, and that every exact-kind case
is exact."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import map_cases as mc
import map_ref as mr
from conftest import REPO

CSRC = os.path.join(REPO, "chore_amd", "csrc")
ENTRY_POINTS = ("chore_gn_stats_bytes", "chore_gn_stats", "chore_gn_relu_fwd", "chore_avgpool2_fwd", "chore_avgpool2_bwd", "chore_upadd_fwd",
                "chore_up2_bwd", "chore_stem_workspace_bytes", "chore_stem_fwd", "chore_stem_x3_workspace_bytes", "chore_stem_x3_fwd",
                "chore_amax_bytes", "chore_absmax_f32")


def _src(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_table_names_exactly_the_entry_points():
    assert len(ENTRY_POINTS) == 13 and set(mc.COVERAGE) == set(ENTRY_POINTS), sorted(set(mc.COVERAGE) ^ set(ENTRY_POINTS))
    text = open(os.path.join(REPO, "chore_amd", "_lib.py")).read()
    names = set(re.findall(r'^\s*"(chore_\w+)"\s*:\s*\(', text, re.M))
    assert set(ENTRY_POINTS) <= names, sorted(set(ENTRY_POINTS) - names)
    header = open(os.path.join(REPO, "include", "chore_hip.h")).read()
    declared = set(re.findall(r"\b(chore_\w+)\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    # no entry point of these operators' families that the table does not know
    family = {n for n in names if re.match(r"chore_(gn_stats|gn_relu_fwd|avgpool2|upadd|up2_bwd|stem_workspace|stem_fwd|stem_x3|amax|absmax)", n)}
    assert family == set(ENTRY_POINTS), sorted(family ^ set(ENTRY_POINTS))


def test_rows_are_case_ids_or_reasons():
    every = {c["id"] for cs in mc.CASES.values() for c in cs}
    assert len(every) == sum(len(cs) for cs in mc.CASES.values()), "duplicate case ids"
    used = set()
    print("coverage table (%d rows):" % len(mc.COVERAGE))
    for name, row in mc.COVERAGE.items():
        if isinstance(row, str):
            assert len(row) > 20 and name.endswith("_bytes"), name
            print("  %-32s %s" % (name, row))
        else:
            assert row and set(row) <= every and len(set(row)) == len(row), name
            used |= set(row)
            print("  %-32s %d cases" % (name, len(row)))
    assert used == every, sorted(every - used)         # no case that reaches no entry point of the table
    # the size functions are called by the test that a reason row names
    text = open(os.path.join(REPO, "tests", "test_gpu_map_kernels.py")).read()
    for name in ENTRY_POINTS:
        assert "L.%s(" % name in text, name
    assert len(mc.OUT_OF_SCOPE) == 3 and all(len(v) > 20 for v in mc.OUT_OF_SCOPE.values())


def test_every_case_family_is_run_by_a_gpu_test():
    text = open(os.path.join(REPO, "tests", "test_gpu_map_kernels.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    run = re.findall(r'@pytest\.mark\.parametrize\("case", mc\.CASES\["(\w+)"\], ids=mc\.ids\("(\w+)"\)\)\ndef (test_\w+)\(case\):', text)
    assert all(a == b for a, b, _ in run), run
    assert sorted(a for a, _, _ in run) == sorted(mc.CASES), (run, sorted(mc.CASES))
    assert "def test_upadd_and_up2_bwd_are_adjoint(size)" in text and len(mc.ADJOINT_HW) == 3
    # the decoder of the statistics cells lives in map_ref.py; the one test that had its own imports it
    assert "from map_ref import stats_cells" in open(os.path.join(REPO, "tests", "test_gpu_train_ops.py")).read()


def test_the_matrix_holds_the_shapes_it_was_asked_for():
    C, K = mc.CASES, mc.CONSTANTS
    vals = lambda fam, key, pred=lambda c: True: {c[key] for c in C[fam] if pred(c)}       # noqa: E731
    sizes = lambda fam, pred=lambda c: True: {(c["H"], c["W"]) for c in C[fam] if pred(c)}    # noqa: E731
    assert {k: len(v) for k, v in C.items()} == {"gn_stats": 58, "gn_relu": 45, "pool": 96, "pool_bwd": 80, "upadd": 42, "up2_bwd": 116, "stem": 56,
                                                 "stem_x3": 30, "absmax": 33, "refused": 48}
    for fam in C:
        if fam != "refused":
            assert vals(fam, "kind") == set(mc.KINDS), fam
    # every random-kind shape has an exact-kind twin
    shape = lambda c: tuple(sorted((k, v) for k, v in c.items() if k in ("B", "C", "H", "W", "HW", "Cin", "dtype", "n", "vec")))      # noqa: E731
    for fam in ("gn_stats", "pool", "pool_bwd", "upadd", "up2_bwd", "stem", "stem_x3", "absmax"):
        assert {shape(c) for c in C[fam] if c["kind"] == "random"} <= {shape(c) for c in C[fam] if c["kind"] == "exact"}, fam
    # gn_stats
    slice_px, slices = K["GN_SLICE_PIXELS"], K["GN_SLICES_MAX"]
    assert vals("gn_stats", "C") == {32, 64, 128, 256} and vals("gn_stats", "B") == {1, 3} and vals("gn_stats", "dtype") == set(mc.DTYPES)
    assert vals("gn_stats", "HW") == {1, slice_px - 1, slice_px, 2 * slice_px + 1, slice_px * slices + 1}
    for kind in mc.KINDS:
        assert len({(c["C"], c["HW"]) for c in C["gn_stats"] if c["dtype"] == "f32" and c["B"] == 3 and c["kind"] == kind}) == 4 * 5
    assert mc.gn_stats_chain(64, slice_px * slices + 1) == (5, 16, slices) and mc.gn_stats_chain(256, 63) == (16, 4, 1)
    # gn_relu
    assert vals("gn_relu", "C") == {32, 64, 128, 256} and vals("gn_relu", "dtype") == set(mc.DTYPES) and vals("gn_relu", "HW") == {1, 100, 4097}
    assert vals("gn_relu", "B") == {1, 3}
    for dt in mc.DTYPES:
        assert len(vals("gn_relu", "C", lambda c: c["dtype"] == dt and c["HW"] == 4097)) == 4
        assert len([c for c in C["gn_relu"] if c["dtype"] == dt and c["stats"] == "device"]) == 1
    assert -(-4097 * (256 // 4) // 256) > K["GN_APPLY_BLOCKS"] >= -(-4097 * (128 // 4) // 256)      # the grid-stride loop runs twice at C = 256 only
    # pool
    T = K["MAP_T"]
    want = {(2, 2), (2 * T, 2 * T), (2 * T + 2, 2 * T - 2), (2, 4 * T + 2)}
    assert sizes("pool") == sizes("pool_bwd") == want
    assert vals("pool", "C") == {64, 128, 256} and vals("pool_bwd", "C") == {4, 36, 64, 128, 256}
    for fam in ("pool", "pool_bwd"):
        assert vals(fam, "B") == {1, 3} and vals(fam, "dtype") == {"f32", "bf16"}
    assert len({(c["C"], c["H"], c["W"], c["B"], c["dtype"], c["kind"]) for c in C["pool"]}) == 3 * 4 * 2 * 2 * 2
    assert len({(c["C"], c["H"], c["W"], c["dtype"], c["kind"]) for c in C["pool_bwd"]}) == 5 * 4 * 2 * 2
    # upadd
    TW = K["UP_TW"]
    assert K["UP_PSX"] == TW // 2 + 4 and K["UP_PS"] == T // 2 + 4
    assert sizes("upadd") == {(1, 1), (2, 2), (2, 3), (T // 2, TW // 2), (T // 2 + 1, TW // 2 + 1), (T // 2, TW // 2 + 1), (12, 17), (128, 3), (3, 128),
                              (255, 2)}
    assert sizes("upadd", lambda c: c["C"] == 64 and c["dtype"] == "f32" and not c["inplace"]) == sizes("upadd")
    assert {(c["C"], c["dtype"]) for c in C["upadd"] if (c["H"], c["W"]) == (5, 9)} == {(c, d) for c in (64, 128, 256) for d in mc.DTYPES}
    assert all(c["C"] == 64 for c in C["upadd"] if (c["H"], c["W"]) in mc.UPADD_LARGE)
    assert vals("upadd", "B") == {1, 3} and {c["dtype"] for c in C["upadd"] if c["inplace"]} == set(mc.DTYPES)
    assert set(mc.ADJOINT_HW) <= sizes("upadd")
    # up2_bwd
    for n in range(2, 21):
        assert {c["W"] for c in C["up2_bwd"] if c["H"] == n and c["C"] == 4} & {2, 3, 7}, n
        assert {c["H"] for c in C["up2_bwd"] if c["W"] == n and c["C"] == 4} & {2, 3, 7}, n
    assert {w for (h, w) in mc.UP2_SIZES[:19]} == {2, 3, 7} and {(128, 3), (3, 128), (255, 2)} <= sizes("up2_bwd", lambda c: c["C"] == 4)
    assert sizes("up2_bwd", lambda c: c["C"] == 4) == set(mc.UP2_SIZES) and vals("up2_bwd", "C") == {4, 64, 256}
    for ch in (64, 256):
        assert len(sizes("up2_bwd", lambda c: c["C"] == ch)) == 3
    assert vals("up2_bwd", "B") == {1, 3} and vals("up2_bwd", "dtype") == {"f32", "bf16"}
    for ch in (4, 64, 256):          # the `live` clamp: a last workgroup with idle threads
        assert any((c["B"] * c["H"] * c["W"] * ch // 4) % 256 for c in C["up2_bwd"] if c["C"] == ch), ch
    # the stems
    ST, SX = K["STEM_T"], K["SX_TW"]
    assert vals("stem", "Cin") == {1, 3, 4, 5, K["STEM_MAXC"]} and vals("stem_x3", "Cin") == {3, 4, 5}
    assert sizes("stem") == {(2, 2), (2 * ST, 2 * ST), (2 * ST + 2, 2 * ST - 2), (22, 18)} and sizes("stem_x3") == sizes("stem") | {(4 * ST, 2 * SX + 2)}
    assert vals("stem", "B") == vals("stem_x3", "B") == {1, 2} and vals("stem", "dtype") == {"f32", "bf16"}
    assert len({(c["Cin"], c["H"], c["W"]) for c in C["stem"] if c["dtype"] == "f32" and c["kind"] == "random"}) == 5 * 4
    assert len({(c["Cin"], c["H"], c["W"]) for c in C["stem_x3"] if c["kind"] == "random"}) == 3 * 5
    # absmax
    U = 8 * K["AMAX_CELLS"] * 256 * 4
    assert mc.ABSMAX_U == U and vals("absmax", "n") == {4, 1024, U - 4, U, U + 4, 2 * U + 1028}
    assert vals("absmax", "place") == set(mc.ABSMAX_PLACES) and vals("absmax", "neg") == {True, False}
    assert vals("absmax", "special") == {None, "denormal", "inf", "zero"}
    assert max(vals("absmax", "n")) * 4 < 17 << 20          # the largest tensor of the matrix
    s = K["AMAX_CELLS"] * 256
    assert mc.absmax_place(U - 4, "first_tail") == s - 1 and mc.absmax_place(U - 4, "last_unrolled") == 8 * s - 2
    assert mc.absmax_place(U, "first_tail") is None and mc.absmax_place(U, "last_unrolled") == 8 * s - 1
    assert mc.absmax_place(U + 4, "first_tail") == 8 * s and mc.absmax_place(2 * U + 1028, "last_unrolled") == 16 * s - 1
    assert mc.absmax_place(2 * U + 1028, "first_tail") == 16 * s and mc.absmax_place(1024, "last_unrolled") is None
    for c in C["absmax"]:
        x = mc.absmax_input(c)
        at = 4 * c["vec"] + c["vec"] % 4
        assert x.size == c["n"] and (c["special"] == "zero" or (np.abs(x[at]) == np.abs(x).max() and (np.abs(x) == np.abs(x[at])).sum() == 1)), c["id"]
    # the refusals the operators owe
    got = {(c["fn"], tuple(sorted(c["over"].items()))) for c in C["refused"]}
    owed = [("chore_gn_stats", dict(C=v)) for v in (0, 16, 288, 96, 160, 192, 224)] + [("chore_gn_stats", d) for d in (dict(B=0), dict(HW=0), dict(dtype=7))]
    owed += [("chore_gn_relu_fwd", d) for d in (dict(C=0), dict(C=-32), dict(C=288), dict(B=0), dict(HW=0))]
    owed += [("chore_avgpool2_fwd", d) for d in (dict(C=32), dict(H=5), dict(dtype="f16"))] + [("chore_avgpool2_bwd", dict(dtype="f16"))]
    owed += [("chore_upadd_fwd", d) for d in (dict(C=32), dict(B=0), dict(H=0), dict(W=0), dict(B=-3), dict(H=-3), dict(W=-3), dict(dtype=7))]
    owed += [("chore_up2_bwd", d) for d in (dict(H=1), dict(C=6), dict(C=0), dict(B=0), dict(dtype="f16"), dict(dtype=7))]
    owed += [("chore_stem_fwd", d) for d in (dict(Cin=9), dict(W=7), dict(dtype="f16"))] + [("chore_stem_x3_fwd", dict(Cin=2)), ("chore_stem_x3_fwd", dict(Cin=6))]
    owed += [("chore_absmax_f32", d) for d in (dict(n=6), dict(misalign=4), dict(null=True))]
    for fn, over in owed:
        assert (fn, tuple(sorted(over.items()))) in got, (fn, over)


def test_constants_are_the_sources():
    K = mc.CONSTANTS
    const = lambda src, name: int(re.search(r"constexpr int (?:\w+ = [\w *+/]+, )*%s = (\d+)" % name, src).group(1))      # noqa: E731
    misc, common = _src("enc_misc.hip"), _src("enc_common.h")
    assert const(misc, "MAP_T") == K["MAP_T"] and const(misc, "STEM_T") == K["STEM_T"] and const(misc, "STEM_MAXC") == K["STEM_MAXC"]
    assert const(misc, "SX_TW") == K["SX_TW"] and const(common, "AMAX_CELLS") == K["AMAX_CELLS"] and const(misc, "NC") == K["UP2_NC"]
    up = misc[misc.index("struct UpAddOp"):misc.index("struct UpAddOp") + 600]
    m = re.search(r"static constexpr int CT = (\d+), TW = (\d+);\s*static constexpr int PS = (\d+), PSX = TW / 2 \+ 4;", up)
    assert m and tuple(int(v) for v in m.groups()) == (K["UP_CT"], K["UP_TW"], K["UP_PS"]) and K["UP_PSX"] == K["UP_TW"] // 2 + 4
    assert "static constexpr int CT = C, TW = MAP_T;" in misc          # PoolOp: all channels, square tiles
    # the launch geometry the shapes rely on
    assert "dim3 grid(((OH + MAP_T - 1) / MAP_T) * ((OW + Op::TW - 1) / Op::TW), B, C / Op::CT);" in misc
    m = re.search(r"int s = HW / (\d+);\s*if \(s < 1\) s = 1;\s*if \(s > (\d+)\) s = (\d+);", misc)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (K["GN_SLICE_PIXELS"], K["GN_SLICES_MAX"], K["GN_SLICES_MAX"])
    m = re.search(r"int blocks = \(int\)\(\(total4 \+ 255\) / 256\);\s*if \(blocks > (\d+)\) blocks = (\d+);", misc)
    assert m and int(m.group(1)) == int(m.group(2)) == K["GN_APPLY_BLOCKS"]
    m = re.search(r"if \(blocks > (\d+)\) blocks = (\d+);\s*\}\s*dim3 grid\(blocks, B\);", misc)
    assert m and int(m.group(1)) == int(m.group(2)) == K["GN_APPLY_BLOCKS_STATS"]
    assert "absmax_f32_kernel, dim3(AMAX_CELLS), dim3(256)" in misc
    assert "const int oy0 = max(0, 2 * ly - 5), ox0 = max(0, 2 * lx - 5);" in misc
    assert "dim3 grid((OW + STEM_T - 1) / STEM_T, (OH + STEM_T - 1) / STEM_T, B);" in misc
    assert "dim3 grid((OW + SX_TW - 1) / SX_TW, (OH + STEM_T - 1) / STEM_T, B);" in misc
    # the loop of absmax_block that map_cases.absmax_place restates
    assert "const size_t stride = (size_t)AMAX_CELLS * 256;" in common and "size_t i = (size_t)blk * 256 + threadIdx.x;" in common
    assert "for (; i + 7 * stride < n4; i += 8 * stride) {" in common and "for (; i < n4; i += stride) {" in common
    # the unit of the statistics cells and the group count that map_ref.py restates
    assert "const double d = (double)x * 0x1p40;" in common and const(common, "GN_GROUPS") == mr.GROUPS
    assert "struct StatCell { unsigned long long lo; long long hi; };" in common and "struct GroupStat { StatCell sum, sq; };" in common
    assert "inline size_t act_stats_bytes(int B) { return (size_t)2 * B * GN_GROUPS * sizeof(GroupStat); }" in common


def test_bicubic_matrix_is_interpolate():
    ns = {n for c in mc.CASES["upadd"] + mc.CASES["up2_bwd"] for n in (c["H"], c["W"])} | {n for s in mc.ADJOINT_HW for n in s}
    assert {1, 2, 3, 20, 128, 255} <= ns
    for n in sorted(ns):
        M = mr.up2_matrix(n)
        eye = torch.eye(n, dtype=torch.float64).reshape(n, 1, n, 1)          # n images of n x 1: column l of M is image l upsampled in y
        want = F.interpolate(eye.expand(n, 1, n, 2 if n == 1 else 1).contiguous(), scale_factor=(2, 1), mode="bicubic", align_corners=True)
        assert np.abs(M - want[:, 0, :, 0].numpy().T).max() <= 1e-12, n
        assert np.abs(M.sum(1) - 1.0).max() <= 1e-12, n
    # both axes at once, and the transpose
    r = mc.rng("bicubic")
    low, dy = r.standard_normal((2, 5, 9, 3)), r.standard_normal((2, 10, 18, 3))
    want = F.interpolate(torch.from_numpy(low).permute(0, 3, 1, 2), scale_factor=2, mode="bicubic", align_corners=True).permute(0, 2, 3, 1).numpy()
    up = mr.upadd(np.zeros_like(dy), low)
    assert np.abs(up - want).max() <= 1e-12
    assert abs((up * dy).sum() - (low * mr.up2_bwd(dy)).sum()) <= 1e-12 * np.abs(up * dy).sum()


def test_window_of_up2_bwd_holds_every_weight():
    """for every n from 2 to 255: the high-resolution coordinates that weigh on low-resolution coordinate l lie in
    max(0, 2 l - 5) ... max(0, 2 l - 5) + 11 -- the claim up2_bwd_kernel's 12 candidates rest on.  They lie in 2 l - 3 ... 2 l + 4 in
    fact: the window has two spare candidates at either end (one of which an fp32 floor at an integer source coordinate may use, with
    a weight of rounding size), so a window that starts at 2 l - 4 computes the same sums; one that starts at 2 l - 2 does not"""
    NC = mc.CONSTANTS["UP2_NC"]
    first, last = NC, -NC
    for n in range(2, 256):
        M = mr.up2_matrix(n)
        for l in range(n):
            rows = np.nonzero(M[:, l])[0]
            o0 = max(0, 2 * l - 5)
            assert rows.size and rows.min() >= o0 and rows.max() <= o0 + NC - 1, (n, l, rows.min(), rows.max())
            first, last = min(first, rows.min() - 2 * l), max(last, rows.max() - 2 * l)
    print("  rows that weigh on l: 2 l %+d ... 2 l %+d" % (first, last))
    assert (first, last) == (-3, 4)


def test_statistics_cells_round_trip():
    r = mc.rng("cells")
    for B in (1, 3):
        s = r.standard_normal((B, 32)) * 10.0 ** r.integers(-6, 7, (B, 32))
        q = np.abs(r.standard_normal((B, 32))) * 10.0 ** r.integers(-6, 9, (B, 32))
        s[0, :4], q[0, :4] = (0.0, -1.0, 2.0 ** 24 - 1, -2.0 ** -40), (0.0, 2.0 ** 40, 0.25, 2.0 ** -40)
        raw = mr.stats_encode(s, q)
        assert raw.dtype == np.uint8 and raw.size == 2 * B * 32 * 32
        ds, dq = mr.stats_decode(raw, B)
        for got, want in ((ds, s), (dq, q)):
            assert np.abs(got - want).max() <= 2.0 ** -41 + 2.0 ** -52 * np.abs(want).max()
        assert np.array_equal(ds[0, :4], s[0, :4]) and np.array_equal(dq[0, :4], q[0, :4])
        # a second encoding of what was decoded is the same bytes; torch tensors decode like arrays
        assert np.array_equal(mr.stats_encode(ds, dq), raw) and np.array_equal(mr.stats_cells(torch.from_numpy(raw)), mr.stats_cells(raw))
    # the device's own form: low limbs that are sums of 32-bit pieces, beyond 2^32
    w = np.zeros((2, 64, 2), np.uint64)
    w[0, 5, 0], w[1, 5, 1] = (3 << 32) + 7, np.int64(-2).view(np.uint64)
    assert mr.stats_cells(w.reshape(-1).view(np.uint8))[5] == ((3 - 2) * 2 ** 32 + 7) / 2 ** 40


def _integers(a, what, unit=1):
    assert np.array_equal(a * unit, np.rint(a * unit)) and np.abs(a * unit).max() < 2 ** 24, what


def test_exact_cases_are_exact():
    """every exact-kind case: reference sums are integers (quarters / sixteenths after the pooling) below 2^24 and reference outputs
    are representable in the case's storage type"""
    n = 0
    for fam, cases in mc.CASES.items():
        for c in cases:
            if c.get("kind") != "exact" or fam == "absmax":
                continue
            n += 1
            dt, unit, stats = c.get("dtype", "f32"), 1, True
            if fam == "gn_stats":
                out = mr.stored(mc.values(c, (c["B"], c["HW"], c["C"])), dt).double().numpy()
            elif fam == "gn_relu":
                gamma, beta = mc.gn_relu_affine(c)
                assert not gamma.any()
                out, stats = np.maximum(beta.astype(np.float64), 0.0), False
            elif fam == "pool":
                out, unit = mr.avgpool2(mr.stored(mc.values(c, (c["B"], c["H"], c["W"], c["C"])), dt).double().numpy()), 4
            elif fam == "pool_bwd":
                out, unit, stats = mr.avgpool2_bwd(mr.stored(mc.values(c, (c["B"], c["H"] // 2, c["W"] // 2, c["C"])), dt).double().numpy()), 4, False
            elif fam == "upadd":
                a, low = (mr.stored(t, dt).double().numpy() for t in mc.upadd_inputs(c))
                assert (c["H"], c["W"]) == (1, 1) or not low.any()
                out = mr.upadd(a, low)
            elif fam == "up2_bwd":
                dy = mr.stored(mc.up2_bwd_input(c), dt).double().numpy()
                out, stats = mr.up2_bwd(dy), False
                assert np.array_equal(out[:, 0, 0], dy[:, 0, 0]) and np.count_nonzero(out) == np.count_nonzero(dy), c["id"]
            else:
                assert fam in ("stem", "stem_x3"), fam
                img, w, bias = mc.stem_inputs(c)
                assert (np.count_nonzero(w.reshape(64, -1), axis=1) == mc.EXACT_STEM_TAPS).all()
                out, stats = mr.stem(img, w, bias)[0], fam == "stem_x3"
            _integers(out, c["id"], unit)
            assert mr.representable(out, dt), c["id"]
            if stats:
                s, q, _ = mr.group_stats(out)
                _integers(s, c["id"] + " sum", unit)
                _integers(q, c["id"] + " sq", unit * unit)
    assert n == sum(len([c for c in cs if c.get("kind") == "exact"]) for f, cs in mc.CASES.items() if f != "absmax")
