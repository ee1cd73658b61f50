"""times the instance-mask rasteriser on render_bench's demo scene: B = 1, setup_renderer's camera, a body-sized ellipsoid at 2.2 m
(group 0) and a sphere of radius 0.3 beside and partly before it (group 1), 30 112 triangles after fill_back, G = 2, 2 x 2 samples
per pixel, at 256, 1024 and 2048 px.  Each side is captured into a graph once; the replays alternate in one process, device events:
  A  chore_instances_fwd: visible + full + face_samples + group_samples, sample_face_index = NULL
  B  the three chore_render_fwd calls it replaces: both meshes, the body alone, the object alone (rgb + depth + alpha each)
and checks that the two sides say the same: sum over groups of A's visible = B's alpha of both, A's full = B's alpha of each alone.
    python scripts/instances_bench.py [replays] [--trace]     (--trace: a few calls of A at 2048 px only, for a kernel trace)"""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from chore_amd import _lib  # noqa: E402
from chore_amd.utils import render_utils as ru  # noqa: E402
from chore_amd.utils.synth import uv_ellipsoid  # noqa: E402
from meshes import icosphere  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f ms  (p10 %.3f, p90 %.3f, min %.3f, max %.3f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


class Side:
    """the buffers and the two graphs of one image size"""

    def __init__(self, tri, grp, S, ssaa, G=2):
        dev, self.h = tri.device, _lib.handle(0)
        B, Fn = tri.shape[:2]
        self.tri, self.grp, self.S, self.ssaa, self.G = tri, grp, S, ssaa, G
        self.ws = torch.empty(_lib.lib.chore_instances_workspace_bytes(B, Fn, G, S, ssaa), dtype=torch.uint8, device=dev)
        self.visible, self.full = torch.empty(B, G, S, S, device=dev), torch.empty(B, G, S, S, device=dev)
        self.face_samples = torch.empty(B, Fn, dtype=torch.int32, device=dev)
        self.group_samples = torch.empty(B, G, 2, dtype=torch.int32, device=dev)
        # the three render calls: the whole list, and each group's faces alone
        self.lists = [tri] + [tri[:, grp[0] == g].contiguous() for g in range(G)]
        self.tex = [torch.ones(B, t.shape[1], 2, 2, 2, 3, device=dev) for t in self.lists]
        self.rws = [torch.empty(_lib.lib.chore_render_workspace_bytes(B, t.shape[1], S, ssaa), dtype=torch.uint8, device=dev)
                    for t in self.lists]
        self.rgb = [torch.empty(B, 3, S, S, device=dev) for _ in self.lists]
        self.depth = [torch.empty(B, S, S, device=dev) for _ in self.lists]
        self.alpha = [torch.empty(B, S, S, device=dev) for _ in self.lists]
        self.bg = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def run_a(self):
        B, Fn = self.tri.shape[:2]
        _lib.check(_lib.lib.chore_instances_fwd(self.h, self.tri.data_ptr(), self.grp.data_ptr(), B, Fn, self.G, self.S, self.ssaa,
                                                0.1, 100.0, self.visible.data_ptr(), self.full.data_ptr(),
                                                self.face_samples.data_ptr(), self.group_samples.data_ptr(), None,
                                                self.ws.data_ptr(), torch.cuda.current_stream().cuda_stream), self.h, "A")

    def run_b(self):
        for t, tex, ws, rgb, depth, alpha in zip(self.lists, self.tex, self.rws, self.rgb, self.depth, self.alpha):
            _lib.check(_lib.lib.chore_render_fwd(self.h, t.data_ptr(), tex.data_ptr(), None, t.shape[0], t.shape[1], 2, self.S,
                                                 self.ssaa, 0.1, 100.0, 1e-3, self.bg, rgb.data_ptr(), depth.data_ptr(),
                                                 alpha.data_ptr(), None, ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       self.h, "B")

    def capture(self, fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        return g


def timed(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    replays = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 60
    trace = "--trace" in sys.argv
    bv, bf = uv_ellipsoid(center=(0.0, 0.0, 2.2))
    sv, sf = icosphere(3, 0.3, (0.3, 0.0, 1.9))
    meshes = [ru.Mesh(v=bv, f=bf), ru.Mesh(v=sv, f=sf)]
    verts, faces = ru.mesh_geometry(meshes, "cuda:0")
    group = ru.mesh_face_group(meshes, "cuda:0")
    for S in ((2048,) if trace else (256, 1024, 2048)):
        r = ru.setup_renderer(image_size=S)
        tri, grp = r._project_faces(verts, faces, (None,) * 5, group)
        side = Side(tri.contiguous(), grp.contiguous(), S, 2)
        if trace:
            for _ in range(10):
                side.run_a()
            torch.cuda.synchronize()
            return
        ga, gb = side.capture(side.run_a), side.capture(side.run_b)
        for _ in range(5):
            ga.replay()
            gb.replay()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(replays):
            ta.append(timed(ga))
            tb.append(timed(gb))
        same = torch.equal(side.visible.sum(1), side.alpha[0]) and all(torch.equal(side.full[:, g], side.alpha[1 + g]) for g in range(2))
        counts = side.group_samples[0].tolist()
        print("%d px, 2x, %d triangles: visible / full samples body %d / %d, object %d / %d; masks equal the three renders' alpha: %s"
              % (S, tri.shape[1], counts[0][0], counts[0][1], counts[1][0], counts[1][1], same), flush=True)
        print("  A  chore_instances_fwd, one walk:            " + stats(ta))
        print("  B  chore_render_fwd x 3 (both, body, object): " + stats(tb))
        print("  median B / median A = %.2f" % (np.median(tb) / np.median(ta)), flush=True)
        if not same:
            raise SystemExit("the masks differ from the renders' alpha")


if __name__ == "__main__":
    main()
