"""times the gradient of the point-to-mesh distance (chore_mesh_dist_bwd, csrc/mesh_dist_bwd.hip) beside its forward
(chore_mesh_dist_fwd) at the sampler's shapes -- body (13 776 faces) and an object of 2 500 faces at 1 x 110 090 and 4 x 20 000
points -- and at the two calls of the fit's interpenetration term at B = 8: the body's 6 890 vertices against the template
and the template's vertices against the body.  Alternating in one process, device events:
  F    the forward with face_idx and closest (the autograd Function asks for face_idx; T below needs closest)
  P    backward alone, dpoints only (the point pass)
  V    backward alone, dverts only  (point pass with records, gather pass, finish pass)
  PV   backward alone, both
  FB   forward + backward through mesh_distance and autograd (both gradients)
  T    the same gradient formed with torch ops on the device from the forward's outputs (index_add_ of the same contributions)
then a short synthetic fit (tests/test_gpu_penetration_term.py's objects at B = 8, recorded graphs): ms per joint iteration
with PENETRATION_TERM off and on, alternating.
    python scripts/mesh_dist_bwd_bench.py [calls] [--trace]   (--trace: a few calls of PV only, for rocprofv3 --kernel-trace --stats)"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from chore_amd import _lib  # noqa: E402
from chore_amd.preprocess import mesh_distance  # noqa: E402
from chore_amd.utils.synth import uv_ellipsoid  # noqa: E402
from mesh_dist_bench import query_points, stats, timed  # noqa: E402
from meshes import icosphere  # noqa: E402


def backward_call(p, v, f, face_idx, closest, dist, g, want_p, want_v):
    """chore_mesh_dist_bwd on preallocated buffers -> a function that launches it"""
    B, N, V, F = p.shape[0], p.shape[1], v.shape[1], f.shape[0]
    dp, dv = torch.empty_like(p), torch.empty_like(v)
    ws = torch.empty(_lib.lib.chore_mesh_dist_bwd_workspace_bytes(B, N, V, F), dtype=torch.uint8, device=p.device)
    h = _lib.handle(p.device.index or 0)

    def run():
        _lib.check(_lib.lib.chore_mesh_dist_bwd(h, p.data_ptr(), v.data_ptr(), f.data_ptr(), face_idx.data_ptr(), closest.data_ptr(),
                                                dist.data_ptr(), g.data_ptr(), B, N, V, F, dp.data_ptr() if want_p else None,
                                                dv.data_ptr() if want_v else None, ws.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), h, "chore_mesh_dist_bwd")
        return dp, dv
    return run


def torch_grads(p, v, f, face_idx, closest, dist, g):
    """dpoints and dverts with tensor ops: the weights of `closest` in its triangle from the plane's normal equations, then
    index_add_ (atomic adds: the order of the sums is not fixed)"""
    B, V = v.shape[0], v.shape[1]
    u = g[..., None] * (p - closest) / dist.clamp_min(1e-30)[..., None]
    tri = f.long()[face_idx.long()]                                               # (B,N,3)
    idx = tri + (torch.arange(B, device=p.device) * V)[:, None, None]
    c = v.reshape(-1, 3)[idx]                                                     # (B,N,3 corners,3)
    ab, ac, aq = c[:, :, 1] - c[:, :, 0], c[:, :, 2] - c[:, :, 0], closest - c[:, :, 0]
    aa, cc, e = (ab * ab).sum(-1), (ac * ac).sum(-1), (ab * ac).sum(-1)
    d1, d2 = (ab * aq).sum(-1), (ac * aq).sum(-1)
    det = (aa * cc - e * e).clamp_min(1e-30)
    b1 = ((cc * d1 - e * d2) / det).clamp(0, 1)
    b2 = torch.minimum(((aa * d2 - e * d1) / det).clamp(0, 1), 1 - b1)
    w = torch.stack([1 - b1 - b2, b1, b2], -1)                                    # (B,N,3)
    dv = torch.zeros(B * V, 3, device=p.device)
    dv.index_add_(0, idx.reshape(-1), (-(w[..., None] * u[:, :, None, :])).reshape(-1, 3))
    return u, dv.reshape(B, V, 3)


def fit_ms_per_joint_iteration(rounds):
    """ms per joint iteration (one outer iteration = steps_per_iter recorded steps) of a short synthetic fit, switch off / on"""
    from test_gpu_penetration_term import _fit_objects
    opt = argparse.Namespace(input_type="RGBM3", norm="group", num_stack=5, num_hourglass=2, hg_down="ave_pool", hourglass_dim=256,
                             skip_hourglass=True, z_feat="xyz", projection_mode="perspective", loadSize=1200, net_img_size=[512, 512],
                             gpu_id=0)
    B = 8
    fitter, net, _, _ = _fit_objects(opt, B=B)
    fitter.use_graphs = fitter.reuse_graphs = True
    fitter.early_stop = False
    ms = {False: [], True: []}
    for r in range(rounds + 1):
        for on in (False, True):
            fitter.PENETRATION_TERM = on
            _, _, _, data = _fit_objects(opt, net=net, B=B)
            fitter.timer = []
            torch.manual_seed(11)
            fitter.optimize_smpl_object(net, data, obj_iter=2, joint_iter=10, steps_per_iter=10, max_iter=10, sil_iter=0)
            torch.cuda.synchronize()
            if r:                                   # round 0 records the graphs
                ms[on] += [e0.elapsed_time(e1) for e0, e1, n, phase in fitter.timer if phase == "joint"]
    fitter.timer = None
    print("synthetic fit, B = %d, template of 642 vertices / 1 280 faces, 10 recorded steps per joint iteration, %d rounds alternating" % (B, rounds))
    for on in (False, True):
        print("  PENETRATION_TERM %-5s ms per joint iteration: %s" % (on, stats(ms[on])))
    print("  the term adds %.3f ms per joint iteration (%.3f ms per step)" % (np.median(ms[True]) - np.median(ms[False]),
                                                                             (np.median(ms[True]) - np.median(ms[False])) / 10))


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 40
    trace = "--trace" in sys.argv
    bv, bf = uv_ellipsoid(center=(0.1, 0.2, 2.2))
    ov, of = icosphere(3, 0.35, (0.45, 0.1, 2.3))
    ov2, of2 = np.concatenate([ov, ov * 0.6 + 0.2]), np.concatenate([of, of + len(ov)])[:2500]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()     # noqa: E731
    P1 = query_points([(bv, bf), (ov, of)], 1, 110090, 0)
    P4 = query_points([(bv, bf), (ov, of)], 4, 20000, 10)
    shift = lambda a, B: np.stack([a + 0.01 * b for b in range(B)])                 # noqa: E731
    shapes = [("body   F=13776", P1, shift(bv, 1), bf), ("body   F=13776", P4, shift(bv, 4), bf),
              ("object F=2500 ", P1, shift(ov2, 1), of2), ("object F=2500 ", P4, shift(ov2, 4), of2),
              ("fit: body vertices against the template F=2500 ", dev(shift(bv, 8), torch.float32), shift(ov2 - 0.3, 8), of2),
              ("fit: template vertices against the body F=13776", dev(shift(ov2 - 0.3, 8), torch.float32), shift(bv, 8), bf)]
    for name, P, vn, fn in shapes:
        v, f = dev(vn, torch.float32), dev(fn, torch.int32)
        B, N = P.shape[0], P.shape[1]
        fwd = lambda: mesh_distance(P, v, f, ("dist", "face_idx", "closest"))      # noqa: E731
        dist, face_idx, closest = fwd()
        g = torch.rand(B, N, device="cuda") + 0.5
        run_p, run_v, run_pv = (backward_call(P, v, f, face_idx, closest, dist, g, wp, wv) for wp, wv in ((1, 0), (0, 1), (1, 1)))
        if trace:
            for _ in range(6):
                run_pv()
            torch.cuda.synchronize()
            continue
        pg, vg = P.clone().requires_grad_(True), v.clone().requires_grad_(True)
        run_fb = lambda: torch.autograd.grad(mesh_distance(pg, vg, f, "dist"), (pg, vg), g)     # noqa: E731
        run_t = lambda: torch_grads(P, v, f, face_idx, closest, dist, g)            # noqa: E731
        for _ in range(3):
            fwd(), run_p(), run_v(), run_pv(), run_fb(), run_t()
        (dp, dv), (tp, tv) = run_pv(), run_t()
        torch.cuda.synchronize()
        print("%s  B=%d N=%d V=%d   max |kernel - tensor ops|: dpoints %.2e  dverts %.2e (|dverts| up to %.1f)"
              % (name, B, N, v.shape[1], float((dp - tp).abs().max()), float((dv - tv).abs().max()), float(dv.abs().max())))
        t = {k: [] for k in ("F", "P", "V", "PV", "FB", "T")}
        for _ in range(calls):
            for k, fn_ in (("F", fwd), ("P", run_p), ("V", run_v), ("PV", run_pv), ("FB", run_fb), ("T", run_t)):
                t[k].append(timed(fn_))
        for k, what in (("F", "forward (dist, face_idx, closest)"), ("P", "backward, dpoints only"), ("V", "backward, dverts only"),
                        ("PV", "backward, both"), ("FB", "forward + backward (autograd)"), ("T", "torch tensor ops, both")):
            print("  %-2s %-34s %s" % (k, what, stats(t[k])))
        print("     backward (both) / forward = %.2f" % (np.median(t["PV"]) / np.median(t["F"])))
        sys.stdout.flush()
    if not trace:
        fit_ms_per_joint_iteration(3)


if __name__ == "__main__":
    main()
