"""times the point-to-mesh distance (chore_mesh_dist_fwd, csrc/mesh_dist.hip) at the shapes of the training-data sampler:
the body blob (6 890 vertices, 13 776 faces) and objects of 1 280 / 2 500 faces at the full frame of the default recipe
(110 090 points) and at train_batch's shape (B = 4, 20 000 points).  Alternating in one process, device events:
  A  chore_mesh_dist_fwd, dist only (record + distance + finish launches)
  V  the same with vert_idx (adds the nearest-vertex launch), as the sampler calls it for the body
  S  chore_mesh_sdf_fwd, dist + winding: the signed call (the same launches, the winding-number sum in the loop)
  T  a chunked tensor-op formulation of the same minimum in torch on the device (what one would write without the kernel)
then BoundarySampler.boundary_sample_all per frame at the default recipe, split into sampling / distances / download.
There is no culling in the kernel, so there is no culling-off variant to compare against.
    python scripts/mesh_dist_bench.py [calls] [--trace]   (--trace: a few calls of V only, for rocprofv3 --kernel-trace --stats)
    python scripts/mesh_dist_bench.py [calls] --only-a    A alone at the six shapes, one JSON line (what --against starts)
    python scripts/mesh_dist_bench.py [calls] --against chore_amd/csrc/build_ab/libchore_hip_<name>.so [--rounds R]
        A of this build against A of another build of the library (scripts/build_variant.sh; chosen through CHORE_HIP_LIB),
        R (default 3) fresh processes of each, alternating: per shape the medians of every process, the spread between the
        processes of ONE build, and the difference between the builds.  A build of an older mesh_dist.hip needs the symbols
        this one exports to load (chore_amd/_lib.py): append stubs of the missing ones to the copy that is compiled."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from chore_amd.preprocess import BoundarySampler, mesh_distance  # noqa: E402
from chore_amd.utils.synth import uv_ellipsoid  # noqa: E402
from meshes import icosphere  # noqa: E402

FLOP_PER_PAIR = 97          # tri_dist2: 62 VALU instructions, an fma counted as 2 (3 edges 14 + 14 + 25, interior 25, shared 19)
# tri_half_angle on top of it: a, b, c 9, cross 9, determinant 6, three squared lengths 15, three dot products 15, denominator 8 = 62
# operations counted as 1 flop each (no fma: -ffp-contract=off), + 3 sqrt and 1 atan2 counted as 1 each although they are many
# instructions -- a count of the arithmetic of the formula, not of the instructions issued
FLOP_PER_PAIR_WINDING = 66
PEAK_FP32_VECTOR = 157.3e12


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f ms  (p10 %.3f, p90 %.3f, min %.3f, max %.3f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def torch_mesh_dist(P, V, F, chunk=1024):
    """the minimum over all triangles of the distance to the nearest of: the three edges, the plane projection where it
    falls inside -- whole-tensor operations, `chunk` points against every triangle at a time"""
    a, b, c = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    ab, ac = b - a, c - a
    aa, cc, e = (ab * ab).sum(-1), (ac * ac).sum(-1), (ab * ac).sum(-1)
    det = aa * cc - e * e
    ok = det > 1e-12 * aa * cc
    inv = torch.where(ok, 1.0 / torch.where(ok, det, torch.ones_like(det)), torch.zeros_like(det))

    def seg(p, s, d):
        t = ((p - s) * d).sum(-1) / (d * d).sum(-1).clamp_min(1e-30)
        r = p - s - t.clamp(0, 1)[..., None] * d
        return (r * r).sum(-1)
    out = torch.empty(P.shape[0], device=P.device)
    for s in range(0, P.shape[0], chunk):
        p = P[s:s + chunk, None]
        q = torch.minimum(torch.minimum(seg(p, a, ab), seg(p, a, ac)), seg(p, b, c - b))
        ap = p - a
        d1, d2 = (ap * ab).sum(-1), (ap * ac).sum(-1)
        v, w = (cc * d1 - e * d2) * inv, (aa * d2 - e * d1) * inv
        r = ap - v[..., None] * ab - w[..., None] * ac
        inside = (v > 0) & (w > 0) & (1 - v - w > 0)
        q = torch.where(inside, torch.minimum(q, (r * r).sum(-1)), q)
        out[s:s + chunk] = q.min(1).values.sqrt()
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def query_points(meshes, B, N, seed):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import mesh_dist_ref as ref
    n = N // 3 + 1
    P = np.stack([ref.sampler_points(meshes, n - n // 101, n // 101, np.random.RandomState(seed + b))[0][:N] for b in range(B)])
    return torch.from_numpy(P).float().cuda()


def against(other, calls, rounds):
    """this build and `other`, `rounds` fresh processes each, alternating; this process never touches the device"""
    runs = {"this": [], "other": []}
    for r in range(rounds):
        for which in ("this", "other"):
            env = dict(os.environ)
            env.pop("CHORE_HIP_LIB", None)
            if which == "other":
                env["CHORE_HIP_LIB"] = os.path.abspath(other)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), str(calls), "--only-a"], env=env, stdout=subprocess.PIPE,
                                 text=True, timeout=300)
            if res.returncode != 0:
                print(res.stdout)
                raise SystemExit("round %d, %s build: exit status %d" % (r, which, res.returncode))
            runs[which].append(json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]))
    print("A (chore_mesh_dist_fwd, dist only): this build against %s, %d processes each, alternating, %d calls per process" %
          (other, rounds, calls))
    ok = True
    for key in runs["this"][0]:
        a, b = np.array([r[key] for r in runs["this"]]), np.array([r[key] for r in runs["other"]])
        spread = max(a.max() - a.min(), b.max() - b.min())
        diff = a.mean() - b.mean()
        within = abs(diff) <= spread
        ok = ok and within
        print("  %-28s this %s  other %s ms | spread of one build %.4f ms, this - other %+.4f ms%s" %
              (key, " ".join("%.4f" % x for x in a), " ".join("%.4f" % x for x in b), spread, diff, "" if within else "  <-- outside"))
    print("A of this build lies within the run-to-run spread of one build at every shape: %s" % ok)


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 40
    trace = "--trace" in sys.argv
    only_a = "--only-a" in sys.argv
    if "--against" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
        return against(sys.argv[sys.argv.index("--against") + 1], calls, rounds)
    medians = {}
    bv, bf = uv_ellipsoid(center=(0.1, 0.2, 2.2))
    ov, of = icosphere(3, 0.35, (0.45, 0.1, 2.3))
    ov2, of2 = icosphere(3, 0.35, (0.45, 0.1, 2.3))
    ov2, of2 = np.concatenate([ov2, ov2 * 0.6 + 0.2]), np.concatenate([of2, of2 + len(ov2)])[:2500]
    meshes = {"body  F=13776": (bv, bf), "object F=1280": (ov, of), "object F=2500": (ov2, of2)}
    P1 = query_points([(bv, bf), (ov, of)], 1, 110090, 0)
    P4 = query_points([(bv, bf), (ov, of)], 4, 20000, 10)
    dev = lambda v, f: (torch.from_numpy(v).float().cuda(), torch.from_numpy(f).int().cuda())     # noqa: E731
    if trace:
        v, f = dev(bv, bf)
        for _ in range(6):
            mesh_distance(P1, v[None], f, ("dist", "vert_idx"))
        torch.cuda.synchronize()
        return
    for name, (vn, fn) in meshes.items():
        v, f = dev(vn, fn)
        for P, B in ((P1, 1), (P4, 4)):
            vb = v[None].expand(B, -1, -1).contiguous()
            N = P.shape[1]
            run_a = lambda: mesh_distance(P, vb, f, "dist")                          # noqa: E731
            run_v = lambda: mesh_distance(P, vb, f, ("dist", "vert_idx"))            # noqa: E731
            run_s = lambda: mesh_distance(P, vb, f, ("dist", "winding"))             # noqa: E731
            if only_a:
                for _ in range(3):
                    run_a()
                torch.cuda.synchronize()
                medians["%s B=%d N=%d" % (name, B, N)] = float(np.median([timed(run_a) for _ in range(calls)]))
                continue
            do_t = B == 1
            run_t = lambda: torch_mesh_dist(P[0], v, f.long())                       # noqa: E731
            for _ in range(3):
                run_a(), run_v(), run_s()
            if do_t:
                got, want = run_a()[0], run_t()
                print("%s: max |kernel - tensor-op formulation| = %.3e" % (name, float((got - want).abs().max())))
            torch.cuda.synchronize()
            ta, tv, ts, tt = [], [], [], []
            for k in range(calls):
                ta.append(timed(run_a))
                tv.append(timed(run_v))
                ts.append(timed(run_s))
                if do_t and k < max(5, calls // 8):
                    tt.append(timed(run_t))
            pairs = B * N * len(fn)
            med = np.median(ta)
            print("%s  B=%d N=%d  (%.3e point-triangle pairs)" % (name, B, N, pairs))
            print("  A  dist:             " + stats(ta))
            print("     %.3e pairs/s, %d flop per pair -> %.1f TFLOP/s = %.1f %% of the %.1f TFLOP/s fp32 vector peak"
                  % (pairs / med * 1e3, FLOP_PER_PAIR, pairs * FLOP_PER_PAIR / med * 1e3 / 1e12,
                     100 * pairs * FLOP_PER_PAIR / med * 1e3 / PEAK_FP32_VECTOR, PEAK_FP32_VECTOR / 1e12))
            print("     run-to-run spread of A (p90 - p10): %.3f ms" % (np.sort(ta)[-1 - len(ta) // 10] - np.sort(ta)[len(ta) // 10]))
            print("  V  dist + vert_idx:  " + stats(tv))
            ms = np.median(ts)
            print("  S  dist + winding:   " + stats(ts) + "   %.2f x A" % (ms / med))
            print("     %d flop per pair -> %.1f TFLOP/s = %.1f %% of the fp32 vector peak"
                  % (FLOP_PER_PAIR + FLOP_PER_PAIR_WINDING, pairs * (FLOP_PER_PAIR + FLOP_PER_PAIR_WINDING) / ms * 1e3 / 1e12,
                     100 * pairs * (FLOP_PER_PAIR + FLOP_PER_PAIR_WINDING) / ms * 1e3 / PEAK_FP32_VECTOR))
            if do_t:
                print("  T  torch tensor ops: " + stats(tt) + "   A is %.0f x faster" % (np.median(tt) / med))
            sys.stdout.flush()
    if only_a:
        print(json.dumps(medians))
        return
    # the sampler per frame: default recipe of preprocess_scale.py
    from chore_amd.preprocess.boundary_sampler import _DeviceMesh

    class M:
        def __init__(self, v, f):
            self.v, self.f = v, f

    class Landmarks:
        def get_smpl_center(self, m):
            return m.v.mean(0)

        def get_body_kpts(self, m):
            return m.v[:25]
    s = BoundarySampler(part_labels=np.random.RandomState(0).randint(0, 14, 6890), seed=0)
    smpl, obj = M(bv, bf), M(ov, of)
    sigmas, ratios = [0.08, 0.02, 0.003], [0.01, 0.49, 0.5]
    for _ in range(2):
        s.boundary_sample_all(Landmarks(), smpl, obj, sigmas, ratios, 100000, grid_ratio=0.01)
    tw = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.boundary_sample_all(Landmarks(), smpl, obj, sigmas, ratios, 100000, grid_ratio=0.01)
        tw.append((time.perf_counter() - t0) * 1e3)
    print("boundary_sample_all, one frame at the default recipe (110 090 points, wall clock): " + stats(tw))
    parts = {"upload": [], "sampling": [], "distances": [], "download": []}
    for _ in range(10):
        def lap(key, t0):
            torch.cuda.synchronize()
            parts[key].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ds, do = _DeviceMesh(smpl, s.device), _DeviceMesh(obj, s.device)
        lap("upload", t0)
        t0 = time.perf_counter()
        pts = [s._draw(ds.vt[None], ds.ft, do.vt[None], do.ft, sg, s.get_sample_num(r, 100000), int(0.01 * s.get_sample_num(r, 100000)),
                       s.generator)[0] for sg, r in zip(sigmas, ratios)]
        lap("sampling", t0)
        t0 = time.perf_counter()
        res = []
        for p in pts:
            d_h, c_h, vid = mesh_distance(p, ds.vt, ds.ft, ("dist", "closest", "vert_idx"))
            d_o, c_o = mesh_distance(p, do.vt, do.ft, ("dist", "closest"))
            res.append(torch.cat([p, d_h[:, None], d_o[:, None], vid[:, None].float(), c_h, c_o], 1))
        lap("distances", t0)
        t0 = time.perf_counter()
        for r in res:
            r.cpu().numpy()
        lap("download", t0)
    for k, v in parts.items():
        print("  %-10s %s" % (k, stats(v)))


if __name__ == "__main__":
    main()
