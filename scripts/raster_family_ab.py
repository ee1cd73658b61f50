#!/usr/bin/env python
"""Two builds of libchore_hip.so against each other on the rasteriser family's benchmarks, on one GPU: fresh processes, old / new /
old / new through CHORE_HIP_LIB (profiles/raster_family_bench.txt).

    python scripts/raster_family_ab.py OLD_LIB NEW_LIB OUT_DIR [--trace [--relist]]

Without --trace: render_bench, render_bwd_bench, splat_bench, scene_bench, instances_bench, sil_time and bench.py --mode fit, each
four times.  Every time a run reports (a `median ... ms` line, sil_time's `ms per forward+backward`, the fit's value) becomes a line
of the table: the old build's two runs give the spread, and the new build's slower run may exceed the old build's slower run by at
most that spread.  The old build is the yardstick.  With --trace: one kernel trace per entry point and build (the scripts' --trace
modes under rocprofv3 --kernel-trace), and the two listings of kernel, grid and workgroup in launch order, compared.
Every child has a time limit; after a child that ends abnormally nothing more is started."""
import csv
import glob
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCHES = [("render_bench", ["scripts/render_bench.py", "20"]), ("render_bwd_bench", ["scripts/render_bwd_bench.py", "20"]),
           ("splat_bench", ["scripts/splat_bench.py", "20"]), ("scene_bench", ["scripts/scene_bench.py", "20"]),
           ("instances_bench", ["scripts/instances_bench.py", "20"]), ("sil_time", ["scripts/sil_time.py"]),
           ("bench_fit", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--mode", "fit"])]
TRACES = [("render_bench", ["scripts/render_bench.py", "--trace"]), ("render_bwd_bench", ["scripts/render_bwd_bench.py", "--trace"]),
          ("splat_bench", ["scripts/splat_bench.py", "--trace"]), ("scene_bench", ["scripts/scene_bench.py", "--trace"]),
          ("instances_bench", ["scripts/instances_bench.py", "--trace"]), ("sil_time", ["scripts/sil_time.py"])]
FAMILY = re.compile(r"sil_|render_|rbw_|splat_|scene_|instances_|raster_")
UNIFIED = re.compile(r"(sil|rbw|render|raster)_setup_kernel(<[^>]*>)?|(splat|scene|instances|raster)_clear_kernel")


def child(cmd, lib, limit, log):
    env = dict(os.environ, CHORE_HIP_LIB=lib)
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=limit)
    with open(log, "w") as f:
        f.write(r.stdout + "\n---- stderr\n" + r.stderr[-4000:])
    if r.returncode:
        sys.exit("%s with %s ended with status %d; nothing more is started\n%s" % (cmd, lib, r.returncode, r.stderr[-2000:]))
    return r.stdout


def times_of(text):
    """[(label, milliseconds)] in the order reported"""
    out = []
    for line in text.splitlines():
        m = re.match(r"\s*(.*?)\s*median (\d+\.\d+) ms", line) or re.match(r"(.*?): (\d+\.\d+) ms per forward\+backward", line)
        if m:
            out.append((m.group(1), float(m.group(2))))
        elif line.startswith("{") and '"value"' in line:
            rec = json.loads(line)
            out.append(("%s [%s]" % (rec.get("metric", "value")[:60], rec.get("unit", "")), float(rec["value"])))
    return [("%s #%d" % (k, i), v) for i, (k, v) in enumerate(out)]


def bench(old, new, out_dir):
    failed = 0
    print("every reported time, ms: old run 1, old run 2, new run 1, new run 2 (run order: old, new, old, new)")
    for name, cmd in BENCHES:
        runs = [times_of(child([sys.executable] + cmd, lib, 400, os.path.join(out_dir, "%s_%s%d.log" % (name, tag, k))))
                for k, (tag, lib) in enumerate((("old", old), ("new", new), ("old", old), ("new", new)))]
        assert [k for k, _ in runs[0]] == [k for k, _ in runs[1]] == [k for k, _ in runs[2]] == [k for k, _ in runs[3]], name
        print("\n---- %s" % " ".join(cmd))
        for i, (label, _) in enumerate(runs[0]):
            o1, n1, o2, n2 = (r[i][1] for r in runs)
            ok = max(n1, n2) - max(o1, o2) <= abs(o1 - o2)
            failed += not ok
            print("%-100s %9.3f %9.3f %9.3f %9.3f   %s" % (label, o1, o2, n1, n2, "ok" if ok else "SLOWER than the old build's spread allows"),
                  flush=True)
    print("\n%d line(s) outside the old build's spread" % failed)


def listing(d):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")),
             "%sx%sx%s" % (r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]),
             "%sx%sx%s" % (r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"])) for r in rows if FAMILY.search(r["Kernel_Name"])]


def trace(old, new, out_dir):
    for name, cmd in TRACES:
        lists = {}
        for tag, lib in (("old", old), ("new", new)):
            d = os.path.join(out_dir, "trace_%s_%s" % (name, tag))
            if "--relist" not in sys.argv:          # --relist: the traces are in OUT_DIR already, only compare and list them
                child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable] + cmd, lib, 400, d + ".log")
            lists[tag] = listing(d)
        a, b = lists["old"], lists["new"]
        same = len(a) == len(b) and all(x[1:] == y[1:] and (x[0] == y[0] or (UNIFIED.fullmatch(x[0]) and UNIFIED.fullmatch(y[0])))
                                        for x, y in zip(a, b))
        print("\n---- %s: %d / %d family kernels, order, grids and workgroups %s" % (" ".join(cmd), len(a), len(b), "EQUAL" if same else "DIFFER"))
        period = next((p for p in range(1, len(a) + 1) if a[-p:] == a[-2 * p:-p] or p == len(a)), len(a))     # the last repeated call
        for x, y in zip(a[-period:], b[-period:]):
            print("  %-44s %-16s %-12s | %-44s %-16s %-12s" % (x + y))


if __name__ == "__main__":
    os.makedirs(sys.argv[3], exist_ok=True)
    (trace if "--trace" in sys.argv else bench)(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]), sys.argv[3])
