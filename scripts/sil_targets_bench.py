"""times the setup of the silhouette term -- the host constructor SilLossROI(...) (np.nonzero boxes, one grid_sample per frame
and mask, scipy's distance_transform_edt per frame) against SilLossROI.from_masks and set_masks (chore_sil_targets,
chore_sil_edge_edt: no host round trip) -- and the edge term's forward and forward + backward (chore_sil_edge_fwd / _bwd), at
B = 1 and 8 frames of 512^2 masks, S = 256.  Every side is timed in a process of its own (`--side`), the processes alternate:
    python scripts/sil_targets_bench.py [calls] [--rounds N]
A call is timed with the host clock around the call and a device synchronise (the host constructor's cost is host work), set_masks
and the edge term also with device events (what a recorded chain pays)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

S = 256
SIDES = ("host", "device", "edge")


def masks(B):
    """B object masks (discs, boxes, ellipses of 512^2 network-input frames) with a person mask overlapping each"""
    yy, xx = np.mgrid[0:512, 0:512]
    obj, person = [], []
    for b in range(B):
        cx, cy, r = 140 + 37 * b, 380 - 29 * b, 40 + 6 * b
        if b % 3 == 0:
            obj.append((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r)
        elif b % 3 == 1:
            obj.append((abs(xx - cx) <= r) & (abs(yy - cy) <= r // 2))
        else:
            obj.append(((xx - cx) / (1.6 * r)) ** 2 + ((yy - cy) / (0.7 * r)) ** 2 <= 1.0)
        person.append((abs(xx - cx - r) <= r // 2) & (abs(yy - cy) <= 2 * r))
    cc = np.array([[1000.0 + 11 * b, 700.0 + 7 * b] for b in range(B)], np.float32)
    return np.stack(person).astype(np.float32), np.stack(obj).astype(np.float32), cc


def wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def run_side(side, B, calls):
    """-> {name: [ms per call]} of one side at one batch size, in this process"""
    import torch
    from chore_amd.recon.obj_pose_roi import SilLossROI
    from fit_harness import template_mesh
    assert torch.cuda.is_available(), "sil_targets_bench needs a GPU"
    mesh = template_mesh()
    person, obj, cc = (torch.from_numpy(a).cuda() for a in masks(B))
    out = {}
    if side == "host":
        build = lambda: SilLossROI(person, obj, mesh, cc, rend_size=S)                    # noqa: E731
        for _ in range(3):
            build()
        out["host constructor (wall)"] = [wall(build, torch) for _ in range(calls)]
    elif side == "device":
        build = lambda: SilLossROI.from_masks(person, obj, mesh, cc, rend_size=S)         # noqa: E731
        for _ in range(3):
            sil = build()
        out["from_masks (wall)"] = [wall(build, torch) for _ in range(calls)]
        refresh = lambda: sil.set_masks(person, obj, cc)                                  # noqa: E731
        for _ in range(3):
            refresh()
        out["set_masks (wall)"] = [wall(refresh, torch) for _ in range(calls)]
        out["set_masks (device events)"] = [events(refresh, torch) for _ in range(calls)]
    else:
        sil = SilLossROI.from_masks(person, obj, mesh, cc, rend_size=S)
        image = (sil.image_ref.roll(5, 2) * sil.keep_mask).contiguous()                   # a silhouette a few pixels off the mask
        fwd = lambda: sil.edge_loss(image)["edge"]                                        # noqa: E731
        leaf = image.clone().requires_grad_(True)

        def fwd_bwd():
            leaf.grad = None
            sil.edge_loss(leaf)["edge"].backward()
        for _ in range(3):
            fwd(), fwd_bwd()
        out["edge term forward (device events)"] = [events(fwd, torch) for _ in range(calls)]
        out["edge term forward + backward (device events)"] = [events(fwd_bwd, torch) for _ in range(calls)]
        out["edge term forward + backward (wall)"] = [wall(fwd_bwd, torch) for _ in range(calls)]
    return out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f ms  (p10 %.3f, p90 %.3f, min %.3f, max %.3f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("calls", nargs="?", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2, help="processes per (side, B), alternating")
    ap.add_argument("--side", choices=SIDES)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    if args.side:           # a child: one side, one batch size, JSON on the last line
        print(json.dumps(run_side(args.side, args.batch, args.calls)))
        return
    res = {}
    for _ in range(args.rounds):
        for B in (1, 8):
            for side in SIDES:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), str(args.calls), "--side", side, "--batch", str(B)],
                                   stdout=subprocess.PIPE, check=True, timeout=300)
                for k, v in json.loads(p.stdout.decode().strip().splitlines()[-1]).items():
                    res.setdefault((B, k), []).append(v)
    for (B, k), runs in res.items():
        print("B = %d  S = %d  %-46s %s   | medians of the %d processes: %s"
              % (B, S, k, stats(sum(runs, [])), len(runs), ", ".join("%.3f" % np.median(r) for r in runs)))


if __name__ == "__main__":
    main()
