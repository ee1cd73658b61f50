"""times the colour / depth renderer on the demo view: B = 1, setup_renderer(image_size=2048), a body-sized ellipsoid at 2.2 m and a
sphere of radius 0.3 beside it (30 112 triangles after fill_back, 4096^2 samples).  Alternating in one process, device events:
  A  chore_render_fwd: rgb + depth + alpha, resolved, sample_face_index = NULL
  B  chore_silhouette_fwd at size = 4096 on the same triangle list (coverage only: the only way to rasterise that list before)
then the 512^2 NrWrapper.render_meshes call end to end (host tensor work and the copy to the host included).
    python scripts/render_bench.py [calls] [--trace]     (--trace: a few calls of A only, for rocprofv3 --kernel-trace --stats)"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from chore_amd import _lib  # noqa: E402
from chore_amd.recon.obj_pose_roi import vertices_to_faces  # noqa: E402
from chore_amd.utils import render_utils as ru  # noqa: E402
from chore_amd.utils.synth import uv_ellipsoid  # noqa: E402
from meshes import icosphere  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f ms  (p10 %.3f, p90 %.3f, min %.3f, max %.3f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 60
    trace = "--trace" in sys.argv
    dev = torch.device("cuda:0")
    h = _lib.handle(0)
    bv, bf = uv_ellipsoid(center=(0.0, 0.0, 2.2))
    sv, sf = icosphere(3, 0.3, (0.6, 0.0, 2.2))
    body, obj = ru.Mesh(v=bv, f=bf), ru.Mesh(v=sv, f=sf)
    nrw = ru.NrWrapper(image_size=2048)
    r = nrw.front_renderer
    verts, faces, texts = nrw.prepare_render([body, obj])
    faces2 = torch.cat((faces, faces.flip(-1)), 1)
    tex2 = torch.cat((texts, texts.permute(0, 1, 4, 3, 2, 5)), 1).contiguous()
    from chore_amd.render import face_light
    light = face_light(vertices_to_faces(verts, faces2), 0.4, 0.3, [1, 1, 1], [1, 1, 1], [1, 0.5, 1]).contiguous()
    tri = vertices_to_faces(r.transform(verts), faces2).contiguous()
    B, Fn = tri.shape[:2]
    S, ssaa = 2048, 2
    ws_a = torch.empty(_lib.lib.chore_render_workspace_bytes(B, Fn, S, ssaa), dtype=torch.uint8, device=dev)
    rgb = torch.empty(B, 3, S, S, device=dev)
    depth, alpha = torch.empty(B, S, S, device=dev), torch.empty(B, S, S, device=dev)
    ws_b = torch.empty(_lib.lib.chore_silhouette_workspace_bytes(B, Fn), dtype=torch.uint8, device=dev)
    fim_b = torch.empty(B, S * ssaa, S * ssaa, dtype=torch.int32, device=dev)
    alpha_b = torch.empty(B, S * ssaa, S * ssaa, device=dev)
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run_a():
        _lib.check(_lib.lib.chore_render_fwd(h, tri.data_ptr(), tex2.data_ptr(), light.data_ptr(), B, Fn, 4, S, ssaa, 0.1, 100.0, 1e-3, bg,
                                             rgb.data_ptr(), depth.data_ptr(), alpha.data_ptr(), None, ws_a.data_ptr(), stream), h, "A")

    def run_b():
        _lib.check(_lib.lib.chore_silhouette_fwd(h, tri.data_ptr(), B, Fn, S * ssaa, 0.1, 100.0, fim_b.data_ptr(), alpha_b.data_ptr(),
                                                 ws_b.data_ptr(), stream), h, "B")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    print("triangles %d, image %d px, %d x %d samples per pixel, workspace %.1f MB" % (Fn, S, ssaa, ssaa, ws_a.numel() / 2 ** 20),
          flush=True)
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
    print("covered share of the frame: %.4f" % float((alpha > 0).float().mean()))
    print("A  chore_render_fwd 2048 px, 2x (rgb + depth + alpha, resolved):  " + stats(ta))
    print("B  chore_silhouette_fwd at 4096 (coverage only):                  " + stats(tb))
    store_mb = S * S * 5 * 4 / 1e6
    print("A stores %.0f MB of resolved outputs; median A = %.1f GB/s of output stores" % (store_mb, store_mb / np.median(ta)))
    # what a user of render_fit_views waits for at 512 px: tensors from numpy meshes, fill_back, light, projection, the launch, the copies back
    nrw5 = ru.NrWrapper(image_size=512)
    for _ in range(3):
        nrw5.render_meshes(nrw5.front_renderer, [body, obj])
    tw = []
    for _ in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nrw5.render_meshes(nrw5.front_renderer, [body, obj])
        tw.append((time.perf_counter() - t0) * 1e3)
    print("NrWrapper.render_meshes 512 px end to end (wall clock):           " + stats(tw))


if __name__ == "__main__":
    main()
