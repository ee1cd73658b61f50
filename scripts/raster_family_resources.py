#!/usr/bin/env python
"""Compiler resource usage of the rasteriser family at two source trees, without a GPU: compiles silhouette.hip, render.hip,
render_bwd.hip, splat.hip, scene.hip and instances.hip of both trees with the flags of chore_amd/build.py plus
-Rpass-analysis=kernel-resource-usage and prints, per kernel, SGPRs, VGPRs, scratch, occupancy and LDS side by side
(profiles/raster_family_resource_usage.txt).  It ends with status 1 if a kernel gains scratch, changes occupancy or LDS, or if the
sets of instantiations differ by more than the kernels named in RENAMED.

    python scripts/raster_family_resources.py OLD_TREE NEW_TREE      (two checkouts of this repository)"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chore_amd.build import FLAGS, HIPCC      # noqa: E402

FILES = ("silhouette.hip", "render.hip", "render_bwd.hip", "splat.hip", "scene.hip", "instances.hip")
# old name -> new name: the setup and clear kernels that became one each
RENAMED = {"sil_setup_kernel": "raster_setup_kernel<0>", "rbw_setup_kernel": "raster_setup_kernel<0>",
           "render_setup_kernel": "raster_setup_kernel<1>", "splat_clear_kernel": "raster_clear_kernel",
           "scene_clear_kernel": "raster_clear_kernel", "instances_clear_kernel": "raster_clear_kernel"}
FIELDS = ("TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def short_name(mangled):
    """kernel<template arguments> of an Itanium name inside the anonymous namespace (integers and bools only)"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    args = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    return name + ("<%s>" % ", ".join(re.findall(r"L[ib](\d+)E", args.group(1))) if args else "")


def usage(tree, fname, tmp):
    src = os.path.join(tree, "chore_amd", "csrc", fname)
    r = subprocess.run([HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, fname + ".o")],
                       capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-3000:])
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(short_name(m.group(1)), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    return out


def main(old_tree, new_tree):
    bad = []
    print("kernel | SGPRs VGPRs scratch[B/lane] occupancy[waves/SIMD] LDS[B/block]   old -> new   (one column where both agree)")
    with tempfile.TemporaryDirectory() as tmp:
        for f in FILES:
            old, new = usage(old_tree, f, tmp), usage(new_tree, f, tmp)
            pairs = [(k, RENAMED.get(k, k)) for k in old]
            lost = [k for k, n in pairs if n not in new]
            # a header's kernel is emitted into every file that includes it, launched there or not (before: render_setup_kernel in
            # render_bwd.hip): the unified kernels may appear in more files than their predecessors did
            extra = [n for n in new if n not in {n for _, n in pairs}]
            added = [n for n in extra if n not in RENAMED.values()]
            print("\n---- %s: %d kernels before, %d after%s" % (f, len(old), len(new), "".join(
                "\n%s | %s   (emitted, not launched from this file)" % (n, " ".join("%d" % new[n][x] for x in FIELDS))
                for n in extra if n not in added)))
            for k, n in sorted(pairs):
                if n not in new:
                    continue
                a, b = [old[k][x] for x in FIELDS], [new[n][x] for x in FIELDS]
                cols = " ".join("%d" % x if x == y else "%d->%d" % (x, y) for x, y in zip(a, b))
                print("%s | %s%s" % (k if k == n else "%s => %s" % (k, n), cols, "" if a[:2] == b[:2] else "      registers differ"))
                if (a[2] == 0 and b[2] != 0) or (k == n and a[2:] != b[2:]) or a[3:] != b[3:]:
                    bad.append((f, k))
            if lost or added:
                bad.append((f, "instantiations lost %s, added %s" % (lost, added)))
    print("\n" + ("NOT EQUAL: %s" % bad if bad else "scratch, occupancy and LDS equal for every kernel; same instantiations apart from the "
                                                       "unified setup and clear kernels"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
