"""times the ordinal depth term of the object fit (csrc/ordinal_depth.hip, SilLossROI.set_occluder / depth_loss) at B = 8 frames,
S = 256, with the real face counts: a 13 776-face body (the occluder) and a 2 500-face template, both windings.
  term      the term's forward + backward through autograd from the step's triangle list and winner map (_OrdinalDepthFn:
            chore_ordinal_depth_fwd / _bwd), and set_occluder once (what a call of optimize_smpl_object pays)
  composed  the same term from rasterize_rgbad depth renders and tensor expressions (clamp, softplus, masks) through autograd:
            with the body's depth rendered every step, and with it rendered once (the body does not move)
  sil_off / sil_on   a 'sil' iteration's rendering terms eagerly, forward + backward to R / t / s: mask_loss alone, and
            mask_loss(parts=True) + depth_loss on the same placement and rasterisation (not a fit iteration: no forward_step,
            no sum_dict, no optimiser step)
Every side is timed in a process of its own (`--side`), the processes alternate:
    python scripts/ordinal_depth_bench.py [calls] [--rounds N]
A call is timed with device events; the 'sil' iterations also with the host clock around the call and a device synchronise
(eager steps are bound by the host's launches)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, S = 8, 256
SIDES = ("term", "composed", "sil_off", "sil_on")


def rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).astype(np.float32)


def scene(torch):
    """the silhouette term of B frames with its occluder set, and a pose under which the template straddles the body's surface"""
    from chore_amd.recon.obj_pose_roi import SilLossROI
    from chore_amd.utils import synth
    bv, bf = synth.uv_ellipsoid()                                      # 6 890 vertices, 13 776 faces
    tv, tf = synth.uv_ellipsoid(25, 50, radii=(0.35, 0.2, 0.12))       # 1 252 vertices, 2 500 faces
    assert len(bf) == 13776 and len(tf) == 2500
    body = np.stack([bv + np.array([0.02 * b, 0.0, 2.4]) for b in range(B)]).astype(np.float32)
    f = 0.8 * 2.4 / 1.7
    K = np.tile(np.array([[f, 0, 0.5], [0, f, 0.5], [0, 0, 1]], np.float32), (B, 1, 1))
    xx = np.arange(S)[None, None, :].repeat(B, 0).repeat(S, 1)
    obj_crop, person_crop = xx >= S // 2, xx < S // 2                  # left half person, right half object
    sil = SilLossROI.from_crops(obj_crop, person_crop, K, tv.astype(np.float32), tf)
    sil.set_occluder(torch.from_numpy(body).cuda(), bf)
    R = torch.from_numpy(np.stack([rot(0.3 + 0.1 * b, 0.2 * b) for b in range(B)])).cuda()
    t = torch.tensor([[0.03, 0.05 * (b % 3), 2.3] for b in range(B)], dtype=torch.float32).cuda()
    s = torch.ones(B).cuda()
    return sil, torch.from_numpy(body).cuda(), bf, R, t, s


def events(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run_side(side, calls):
    """-> {name: [ms per call]} of one side, in this process"""
    import torch
    import torch.nn.functional as F
    from chore_amd.recon.obj_pose_roi import DEPTH_CLAMP, FAR, NEAR, _OrdinalDepthFn
    from chore_amd.render.renderer import rasterize_rgbad
    assert torch.cuda.is_available(), "ordinal_depth_bench needs a GPU"
    sil, body, bf, R, t, s = scene(torch)
    out = {}
    with torch.no_grad():
        _, tri, fim = sil.render_parts(R, t, s)
    info = sil.depth_order_counts(R, t, s).sum(0).tolist()
    if side == "term":
        leaf = tri.clone().requires_grad_(True)

        def fwd():
            return _OrdinalDepthFn.apply(leaf, fim, sil.occ_depth, sil.image_ref, sil.keep_mask, DEPTH_CLAMP).mean()

        def fwd_bwd():
            leaf.grad = None
            fwd().backward()
        occl = lambda: sil.set_occluder(body, bf)                                   # noqa: E731
        for _ in range(5):
            fwd(), fwd_bwd(), occl()
        out["term forward (device events)"] = [events(fwd, torch) for _ in range(calls)]
        out["term forward + backward (device events)"] = [events(fwd_bwd, torch) for _ in range(calls)]
        out["set_occluder, once per call (device events)"] = [events(occl, torch) for _ in range(calls)]
    elif side == "composed":
        leaf = tri.clone().requires_grad_(True)
        occ_tri = sil._occ_tri
        tex_o = torch.zeros(B, tri.shape[1], 2, 2, 2, 3, device="cuda")
        tex_h = torch.zeros(B, occ_tri.shape[1], 2, 2, 2, 3, device="cuda")
        O = sil.image_ref > 0.5
        P = ~O & (sil.keep_mask < 0.5)

        def body_depth():
            with torch.no_grad():
                return rasterize_rgbad(occ_tri, tex_h, None, S, False, NEAR, FAR)["depth"]
        d_h_once = body_depth()

        def term(d_h):
            d_o = rasterize_rgbad(leaf, tex_o, None, S, False, NEAR, FAR)["depth"]
            both = (d_o < FAR) & (d_h < FAR)
            a = P & both & (d_o < d_h)
            b = O & both & (d_h < d_o)
            terms = a * F.softplus(torch.clamp(d_h - d_o, max=DEPTH_CLAMP)) + b * F.softplus(torch.clamp(d_o - d_h, max=DEPTH_CLAMP))
            return terms.sum((1, 2)).mean()

        def per_step():
            leaf.grad = None
            term(body_depth()).backward()

        def once():
            leaf.grad = None
            term(d_h_once).backward()
        for _ in range(5):
            per_step(), once()
        out["composed forward + backward, body depth per step (device events)"] = [events(per_step, torch) for _ in range(calls)]
        out["composed forward + backward, body depth once (device events)"] = [events(once, torch) for _ in range(calls)]
        with torch.no_grad():                                                                # same inputs, same term
            want = _OrdinalDepthFn.apply(tri, fim, sil.occ_depth, sil.image_ref, sil.keep_mask, DEPTH_CLAMP).mean()
            info.append(float((term(d_h_once) - want).abs() / want.abs().clamp_min(1e-30)))
    else:
        on = side == "sil_on"
        pR, pt, ps = (x.clone().requires_grad_(True) for x in (R, t, s))

        def step():
            for p in (pR, pt, ps):
                p.grad = None
            if on:
                loss, _, tri_, fim_ = sil.mask_loss(pR, pt, ps, parts=True)
                total = loss["mask"] + sil.depth_loss(tri_, fim_)["depth"]
            else:
                total = sil.mask_loss(pR, pt, ps)[0]["mask"]
            total.backward()
        for _ in range(5):
            step()
        name = "'sil' rendering terms, switch %s" % ("on" if on else "off")
        out[name + " (device events)"] = [events(step, torch) for _ in range(calls)]
        out[name + " (wall)"] = [wall(step, torch) for _ in range(calls)]
    out["_info"] = info
    return out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f ms  (p10 %.3f, p90 %.3f, min %.3f, max %.3f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("calls", nargs="?", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=2, help="processes per side, alternating")
    ap.add_argument("--side", choices=SIDES)
    args = ap.parse_args()
    if args.side:           # a child: one side, JSON on the last line
        print(json.dumps(run_side(args.side, args.calls)))
        return
    res, info = {}, {}
    for _ in range(args.rounds):
        for side in SIDES:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), str(args.calls), "--side", side], stdout=subprocess.PIPE,
                               check=True, timeout=280)
            for k, v in json.loads(p.stdout.decode().strip().splitlines()[-1]).items():
                if k == "_info":
                    info[side] = v
                else:
                    res.setdefault(k, []).append(v)
    print("B = %d  S = %d  body 13 776 faces, template 2 500 faces (both windings)" % (B, S))
    print("pixels of the scene in case A / case B / person & both / object & both: %s" % info["term"][:4])
    print("composed term against the kernel's on the same inputs, relative difference: %.3e" % info["composed"][4])
    for k, runs in res.items():
        print("%-72s %s   | medians of the %d processes: %s" % (k, stats(sum(runs, [])), len(runs), ", ".join("%.3f" % np.median(r) for r in runs)))


if __name__ == "__main__":
    main()
