"""CPU: which kernel and tiling every convolution launch gets -- conv_launch_plan (csrc/conv_plan.h; no handle, no device) against
the literal expectations of tests/conv_plan_cases.py, recorded on an MI355X at the commit before the plan existed.

The plan's switches are read once per process, so each switch set runs tests/conv_plan_sweep.cpp -- the header alone, built with the
host compiler and -fsanitize=address,undefined as an executable of its own -- under that set's environment; the default set is also
asked of the library in-process (chore_conv_plan).  A coarse grid over every mode, taps, batch, map size, channel count and trait
combination must run clean under the sanitizers and stay inside the launchers' instantiation tables."""
import ctypes
import os
import re

import pytest

import conv_cases as cc
import conv_plan_cases as pc


def _lines(jobs):
    return [" ".join(str(v) for v in pc.plan_args(c, m)) for c, m in jobs]


@pytest.mark.parametrize("name", list(cc.SWITCH_SETS))
def test_plan_of_every_job(name):
    jobs, want = cc.jobs_of(name), pc.EXPECTED[name]
    assert [(c["id"], m) for c, m in jobs] == [(cid, m) for cid, m, _ in want]
    got = pc.sweep(cc.SWITCH_SETS[name][0], _lines(jobs))
    assert len(got) == len(jobs)
    bad = []
    for (c, m), (_, _, rec), line in zip(jobs, want, got):
        if line != "%d %d %d %d %d %d %d" % (rec + (pc.CLASS_NAMES.index(pc.class_name(c, rec)),)):
            bad.append("%s %s: the plan says '%s', the launch was %r (class %s)" % (c["id"], m, line, rec, pc.class_name(c, rec)))
    assert not bad, "\n".join(["%d of %d jobs" % (len(bad), len(jobs))] + bad[:40])


def test_library_gives_the_default_set_in_process():
    from chore_amd import _lib
    assert not [k for k in pc.SWITCH_NAMES if k in os.environ], "this test reads the plan under the process's own switches: none may be set"
    for (c, m), (_, _, rec) in zip(cc.jobs_of("default"), pc.EXPECTED["default"]):
        out = (ctypes.c_int * 8)()
        assert _lib.lib.chore_conv_plan(*pc.plan_args(c, m), out, 8) == 7
        assert tuple(out[:7]) == rec + (pc.CLASS_NAMES.index(pc.class_name(c, rec)),), (c["id"], m, list(out))
    assert _lib.lib.chore_conv_plan(*pc.plan_args(c, m), None, 8) == -1      # CHORE_EINVAL: nowhere to write


def test_refused_combinations():
    from chore_amd import _lib
    got = pc.sweep({}, [" ".join(str(v) for v in args) for args, _ in pc.REFUSED])
    assert got == ["refused: " + text for _, text in pc.REFUSED]
    out = (ctypes.c_int * 8)()
    for args, text in pc.REFUSED:
        assert _lib.lib.chore_conv_plan(*args, out, 8) == -1, (args, text)       # CHORE_EINVAL


def test_class_names_are_the_encoders():
    src = open(os.path.join(pc.REPO, "chore_amd", "csrc", "encoder.hip")).read()
    names = re.findall(r'"([^"]+)"', re.search(r"kclass_names\[K_NUM\] = \{(.*?)\};", src, re.S).group(1))
    assert tuple(names[-len(pc.CLASS_NAMES):]) == pc.CLASS_NAMES and names[-len(pc.CLASS_NAMES) - 1] == "map_stats_kernel<T,C,UpAddOp>"


def check_in_tables(rows):
    for mode, taps, scaled, fam, th, nt, tps, nslot, small_grid, cin in rows:
        row = (mode, taps, scaled, fam, th, nt, tps, nslot, small_grid, cin)
        dt = "x3s" if mode == "x3" and scaled else mode
        assert not scaled or mode == "x3" or fam in (1, 2, 3), row       # (the trait is ignored outside fp16 x 3: never conv_mw / conv_rw)
        if fam == 1:
            assert th == 8 and nslot == 2 and tps == (1 if taps == 1 else (9 if small_grid else 3)), row
            assert nt in ((128, 64, 32) if mode == "bf16" else (64, 32)) and mode != "fp16", row
            assert not small_grid or (mode in ("fp32", "bf16") and nt <= 64), row
        elif fam == 2:
            assert taps == 9 and th in cc.SMALL_ROWS and cin in (64, 128, 256) and mode != "fp32" and (nt, tps, nslot) == (32, 9, 0), row
            assert ("small", dt if mode == "x3" else mode, cin, th) in cc.COVERAGE, row
        elif fam == 3:
            assert (taps, th, nt, tps, nslot) in cc.PC_TILINGS and mode != "fp32", row
        elif fam == 4:
            assert taps == 9 and mode == "x3" and (th, nt, tps, nslot) in cc.MW_TILINGS, row
        else:
            assert fam == 5 and taps == 1 and (cin, nt) in cc.RW_SHAPES and (th, tps, nslot) == (0, 1, 0) and mode != "fp32", row
            assert not scaled or (mode == "x3" and (cin, nt) == (256, 256)), row


@pytest.mark.parametrize("force", [cc.SWITCH_SETS["pc_force"][0]["CHORE_PC_FORCE"], "9,64,64:4064;;x,;9,64"], ids=["pc_force", "malformed"])
def test_grid_stays_inside_the_instantiation_tables(force):
    rows, refused = pc.grid_rows(force)
    assert len(rows) > 60 and refused > 0
    check_in_tables(rows)
    fams = {r[3] for r in rows}
    assert fams == {1, 2, 3, 4, 5}, fams
