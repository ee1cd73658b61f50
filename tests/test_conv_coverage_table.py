"""CPU: the coverage table of tests/test_gpu_conv_kernels.py (conv_cases.COVERAGE) names every instantiation the convolution
launchers can pick.  The PC_CASE / MW_CASE / RW_CASE lines and the rows switch of launch_small_r are parsed out of the sources: a
new instantiation without a row in the table -- hence without a matrix case, or without a written reason -- fails here, before
anyone reaches a GPU.  What the planner picks is asked of the plan itself (csrc/conv_plan.h through tests/conv_plan_sweep.cpp)."""
import os
import re

import conv_cases as cc
import conv_plan_cases as pc
from conftest import REPO

CSRC = os.path.join(REPO, "chore_amd", "csrc")


def _src(name):
    s = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", s)


def _calls(src, macro):
    """argument tuples of `MACRO(1, 2, ...);` uses (the #define line has names, not numbers, and does not match)"""
    return [tuple(int(v) for v in m.group(1).split(",")) for m in re.finditer(r"\b%s\(\s*([0-9][0-9,\s]*)\)\s*;" % macro, src)]


def test_table_names_every_conv_pc_tiling():
    got = _calls(_src("conv_pc.hip"), "PC_CASE")
    assert len(got) == 7 and sorted(got) == sorted(cc.PC_TILINGS), got
    for t in got:
        for dt in ("fp16", "bf16", "x3", "x3s"):        # launch_conv_pc instantiates every tiling for h16_t, bf16_t, x3_t and x3_t scaled
            # every conv_pc tiling ships (conv_pc_tile names each one), so each must be reached, not explained away
            assert cc.COVERAGE.get(("pc", dt) + t, "") is None, (dt, t)
    # ... and the plan (csrc/conv_plan.h) reaches every (rows, channels) pair of them, with the ring the PC_CASE line names, over the
    # grid of tests/conv_plan_sweep.cpp; 4 x 32 x 64 only where CHORE_PC_FORCE asks for it (conv_cases.SWITCH_SETS, "pc_force")
    rows, _ = pc.grid_rows(cc.SWITCH_SETS["pc_force"][0]["CHORE_PC_FORCE"])
    planned = {(r[1],) + r[4:8] for r in rows if r[3] == 3}
    assert planned == set(got), planned
    assert {t[1:3] for t in planned} == {(8, 128), (8, 64), (8, 32), (4, 64), (4, 32)}
    assert (9, 4, 64, 3, 2) not in {(r[1],) + r[4:8] for r in pc.grid_rows("")[0] if r[3] == 3}
    src = _src("conv_pc.hip")
    assert "launch_pc_t<h16_t" in src and "launch_pc_t<bf16_t" in src and src.count("launch_pc_t<x3_t") == 2


def test_table_names_every_conv_mw_tiling():
    got = _calls(_src("conv_mw.hip"), "MW_CASE")
    assert len(got) == 8 and sorted(got) == sorted(cc.MW_TILINGS), got
    for t in got:
        for v in ("gn", "scaled"):
            assert cc.COVERAGE.get(("mw", v) + t, "") is None, (v, t)     # every conv_mw tiling ships: each must be reached


def test_table_names_every_conv_rw_shape():
    src = _src("conv_rw.hip")
    got = [(kc, 32 * wn) for kc, wn in _calls(src, "RW_CASE")]
    assert len(got) == 3 and sorted(got) == sorted(cc.RW_SHAPES), got
    for cin, cout in got:
        for dt in ("x3", "fp16", "bf16"):
            assert cc.COVERAGE.get(("rw", dt, cin, cout, ""), "") is None, (dt, cin, cout)
            assert ("rw", dt, cin, cout, "res") in cc.COVERAGE
    # the scaled data gradient: one shape, outside the macro
    assert re.search(r"k == 256 && n == 256\) return res \? launch_rw_t<T, 256, 8, true, true>", src)
    assert cc.COVERAGE.get(("rw", "x3s", 256, 256, ""), "") is None


def test_table_names_every_conv_small_instantiation():
    src = _src("conv_small.hip")
    body = re.search(r"int launch_small_r\(.*?\{(.*?)\n\}", src, re.S).group(1)
    rows = sorted(int(m.group(1)) for m in re.finditer(r"case (\d+):", body))
    assert rows == sorted(cc.SMALL_ROWS), rows
    body = re.search(r"int launch_small_c\(.*?\{(.*?)\n\}", src, re.S).group(1)
    cins = sorted(int(m.group(1)) for m in re.finditer(r"case (\d+):", body))
    assert cins == [64, 128, 256], cins
    types = sorted(set(re.findall(r"launch_small_c<(\w+)>", src)))
    assert types == ["bf16_t", "h16_t", "x3_t", "x3s_t"], types
    for dt in ("bf16", "fp16", "x3", "x3s"):
        for cin in cins:
            for r in rows:
                assert ("small", dt, cin, r) in cc.COVERAGE, (dt, cin, r)
            # the rows a default process picks must be reached
            assert cc.COVERAGE[("small", dt, cin, cc.SMALL_DEFAULT_ROWS[dt])] is None
    # ... and they are what the plan says (csrc/conv_plan.h, conv_small_rows): 2 rows for the 32 x 32 maps with fp16 operands, 1 with
    # bf16 (the larger maps default to 0 = not this kernel), halved while the patch does not fit the LDS: (rows + 2) x PW pixels x
    # (2 Cin + 16) bytes per plane, two planes for fp16 x 3, + 8 Cin + 2048 bytes, in 160 KB.  Asked of the plan for the default and
    # for every number of rows CHORE_CONV_SMALL_ROWS32 can ask for
    pw = int(re.search(r"constexpr int PW = (\d+);", src).group(1))
    assert pw == int(re.search(r"constexpr int CONV_SMALL_PW = (\d+);", open(os.path.join(CSRC, "conv_plan.h")).read()).group(1))

    def fits(dt, cin, r):
        while r > 0 and (2 if dt in ("x3", "x3s") else 1) * (r + 2) * pw * (cin * 2 + 16) + cin * 8 + 2048 > 160 * 1024:
            r >>= 1
        return r
    jobs = [(dt, cin) for dt in ("bf16", "fp16", "x3", "x3s") for cin in cins]
    lines = ["%d 9 4 32 32 %d 64 %d 0" % (pc.DTYPE[dt[:2] if dt == "x3s" else dt], cin, pc.TRAIT_OUT | (pc.TRAIT_SCALED if dt == "x3s" else pc.TRAIT_GN))
             for dt, cin in jobs]
    for asked in (None, 1, 2, 4):
        got = pc.sweep({} if asked is None else {"CHORE_CONV_SMALL_ROWS32": str(asked)}, lines)
        for (dt, cin), line in zip(jobs, got):
            want = fits(dt, cin, asked if asked else (1 if dt == "bf16" else 2))
            assert [int(v) for v in line.split()][:5] == [2, want, 32, 9, 0], (dt, cin, asked, line)
            if asked is None:
                assert want == cc.SMALL_DEFAULT_ROWS[dt], (dt, cin, want)
    # the 64 x 64 maps: not this kernel unless a switch asks
    assert all(int(l.split()[0]) != 2 for l in pc.sweep({}, [l.replace(" 32 32 ", " 64 64 ") for l in lines]))
    assert all(l.split()[:2] == ["2", "1"] for l in pc.sweep({"CHORE_CONV_SMALL_ROWS64": "1", "CHORE_CONV_SMALL_ROWS64_C256": "1"},
                                                             [l.replace(" 32 32 ", " 64 64 ") for l in lines]))


def test_table_rows_are_covered_or_explained():
    assert len(cc.COVERAGE) > 100
    for k, why in cc.COVERAGE.items():
        assert why is None or len(why) > 20, k
    # conv_lds_kernel: what launch_nt can return for the modes conv_lds_nt serves
    for dt, nts in (("fp32", (64, 32)), ("bf16", (128, 64, 32)), ("x3", (64, 32)), ("x3s", (64, 32))):
        for taps in (1, 9):
            for nt in nts:
                assert ("lds", dt, taps, nt, False) in cc.COVERAGE
    # every case of the matrix runs in at least one switch set, and every switch set has cases
    ran = set()
    for name in cc.SWITCH_SETS:
        jobs = cc.jobs_of(name)
        assert jobs, name
        ran |= {c["id"] for c, _ in jobs}
    assert ran == {c["id"] for c in cc.cases()}
