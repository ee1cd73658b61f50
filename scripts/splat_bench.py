"""times the point rasteriser at the debug view's size: B = 1, image_size = 2048, 2 x 2 samples, under the Kinect K, around z = 2.2:
5 000 + 5 000 generator points of 8 mm world radius, 6 890 vertices of 5 mm, two 6 cm markers (16 892 points, 4096^2 samples).
Alternating in one process, device events:
  A  chore_splat_fwd: rgb + depth + alpha, resolved, sample_point_index = NULL
  B  chore_render_fwd of scripts/render_bench.py's ellipsoid scene at the same size (the mesh render of the same frame)
    python scripts/splat_bench.py [calls] [--trace]     (--trace: a few calls of A only, for rocprofv3 --kernel-trace --stats)"""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from chore_amd import _lib  # noqa: E402
from chore_amd.recon.obj_pose_roi import vertices_to_faces  # noqa: E402
from chore_amd.render import face_light, world_radius_to_pixels  # noqa: E402
from chore_amd.utils import render_utils as ru  # noqa: E402
from chore_amd.utils.synth import uv_ellipsoid  # noqa: E402
from meshes import icosphere  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f ms  (p10 %.3f, p90 %.3f, min %.3f, max %.3f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def debug_clouds(seed=0):
    """(points (N,3), colours (N,3), world radii (N,)): two generator-like clouds, a vertex-like cloud, two markers"""
    rs = np.random.RandomState(seed)
    human = rs.normal(0, 1, (5000, 3)) * (0.25, 0.55, 0.15) + (0.0, 0.0, 2.2)
    obj = rs.normal(0, 1, (5000, 3)) * (0.2, 0.2, 0.2) + (0.6, 0.1, 2.2)
    d = rs.normal(0, 1, (6890, 3))
    verts = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.25, 0.85, 0.15) + (0.0, 0.0, 2.2)
    marks = np.array([[0.0, 0.0, 2.2], [0.6, 0.1, 2.2]])
    pts = np.concatenate([human, obj, verts, marks]).astype(np.float32)
    col = np.concatenate([ru.PART_COLORS[rs.randint(0, 14, 5000)], np.tile([[1.0, 0, 0]], (5000, 1)), np.tile([[0, 1.0, 0]], (6890, 1)),
                          [[1.0, 1.0, 0], [0, 1.0, 1.0]]]).astype(np.float32)
    rad = np.concatenate([np.full(10000, 0.008), np.full(6890, 0.005), np.full(2, 0.06)]).astype(np.float32)
    return pts, col, rad


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 60
    trace = "--trace" in sys.argv
    dev = torch.device("cuda:0")
    h = _lib.handle(0)
    S, ssaa, B = 2048, 2, 1
    nrw = ru.NrWrapper(image_size=S)
    r = nrw.front_renderer
    pts, col, rad = (torch.from_numpy(a).to(dev) for a in debug_clouds())
    ndc = r.transform(pts[None]).contiguous()
    rad_px = world_radius_to_pixels(rad[None], ndc[..., 2], float(r.focal_pixels())).contiguous()
    col = col[None].contiguous()
    N = ndc.shape[1]
    ws_a = torch.empty(_lib.lib.chore_splat_workspace_bytes(B, N, S, ssaa), dtype=torch.uint8, device=dev)
    out_a = [torch.empty(B, 3, S, S, device=dev), torch.empty(B, S, S, device=dev), torch.empty(B, S, S, device=dev)]
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # B: the mesh scene of render_bench.py
    bv, bf = uv_ellipsoid(center=(0.0, 0.0, 2.2))
    sv, sf = icosphere(3, 0.3, (0.6, 0.0, 2.2))
    verts, faces, texts = nrw.prepare_render([ru.Mesh(v=bv, f=bf), ru.Mesh(v=sv, f=sf)])
    faces2 = torch.cat((faces, faces.flip(-1)), 1)
    tex2 = torch.cat((texts, texts.permute(0, 1, 4, 3, 2, 5)), 1).contiguous()
    light = face_light(vertices_to_faces(verts, faces2), 0.4, 0.3, [1, 1, 1], [1, 1, 1], [1, 0.5, 1]).contiguous()
    tri = vertices_to_faces(r.transform(verts), faces2).contiguous()
    Fn = tri.shape[1]
    ws_b = torch.empty(_lib.lib.chore_render_workspace_bytes(B, Fn, S, ssaa), dtype=torch.uint8, device=dev)
    out_b = [torch.empty(B, 3, S, S, device=dev), torch.empty(B, S, S, device=dev), torch.empty(B, S, S, device=dev)]

    def run_a():
        _lib.check(_lib.lib.chore_splat_fwd(h, ndc.data_ptr(), col.data_ptr(), rad_px.data_ptr(), 0.0, B, N, S, ssaa, 0.6, 0.1, 100.0, bg,
                                            out_a[0].data_ptr(), out_a[1].data_ptr(), out_a[2].data_ptr(), None, ws_a.data_ptr(),
                                            stream), h, "A")

    def run_b():
        _lib.check(_lib.lib.chore_render_fwd(h, tri.data_ptr(), tex2.data_ptr(), light.data_ptr(), B, Fn, 4, S, ssaa, 0.1, 100.0, 1e-3, bg,
                                             out_b[0].data_ptr(), out_b[1].data_ptr(), out_b[2].data_ptr(), None, ws_b.data_ptr(),
                                             stream), h, "B")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    rs = rad_px[0] * ssaa
    print("points %d, image %d px, %d x %d samples per pixel, key buffer %.1f MB; radius in samples: median %.1f, max %.1f"
          % (N, S, ssaa, ssaa, ws_a.numel() / 1e6, float(rs.median()), float(rs.max())), flush=True)
    if trace:
        for _ in range(10):
            run_a()
        torch.cuda.synchronize()
        return
    for _ in range(5):
        run_a()
        run_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(calls):
        ta.append(timed(run_a))
        tb.append(timed(run_b))
    cover = float((out_a[2] > 0).float().mean())
    print("covered share of the frame: splats %.4f, meshes %.4f" % (cover, float((out_b[2] > 0).float().mean())))
    print("A  chore_splat_fwd 2048 px, 2x (rgb + depth + alpha, resolved):   " + stats(ta))
    print("B  chore_render_fwd 2048 px, 2x, 30 112 triangles, same process:  " + stats(tb))
    keys_mb, store_mb = ws_a.numel() / 1e6, S * S * 5 * 4 / 1e6
    total = 2 * keys_mb + store_mb          # the keys written once and read once, the resolved outputs written once
    print("A moves at least %.0f MB (keys cleared %.0f + read %.0f, outputs %.0f): %.3f ms at the 8 TB/s peak, %.3f ms at the 6.3 TB/s a "
          "copy reaches; median A = %.2f TB/s of that" % (total, keys_mb, keys_mb, store_mb, total / 8e3, total / 6.3e3,
                                                                      total / np.median(ta) / 1e3))


if __name__ == "__main__":
    main()
