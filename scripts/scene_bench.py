"""times the scene rasteriser on scripts/splat_bench.py's frame: its ellipsoid meshes (30 112 triangles with both windings, opacity
0.6) and its debug clouds (16 892 points), B = 1, 2 x 2 samples, at image_size 2048 (demo.py's view) and 512 (the fit's debug view).
Alternating in one process, device events, 5 warm-up rounds:
  A  chore_scene_fwd: both layers composed per sample, resolved once
  B  chore_render_fwd, then chore_splat_fwd: the same passes without composition (two resolves, two sets of outputs)
  C  the layered composition tests/test_gpu_scene.py uses as its oracle: both calls at twice the size with ssaa = 1, then the select
     and the 2 x 2 pooling in torch (opaque faces: a select; the per-sample layers go through memory)
  D  chore_scene_layers_fwd on A's inputs with the mesh index as face group, K = 2, 4 and 8 (reported as D over A)
    python scripts/scene_bench.py [calls] [--trace]     (--trace: a few calls of A at 2048 only, for rocprofv3 --kernel-trace --stats)"""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from chore_amd import _lib  # noqa: E402
from chore_amd.recon.obj_pose_roi import vertices_to_faces  # noqa: E402
from chore_amd.render import face_light, world_radius_to_pixels  # noqa: E402
from chore_amd.utils import render_utils as ru  # noqa: E402
from chore_amd.utils.synth import uv_ellipsoid  # noqa: E402
from meshes import icosphere  # noqa: E402
from splat_bench import debug_clouds, stats  # noqa: E402

NEAR, FAR, EPS, AMBIENT, BIAS, OPACITY = 0.1, 100.0, 1e-3, 0.6, 0.02, 0.6


class Frame:
    """the inputs of one image size and the variants on buffers allocated up front"""

    def __init__(self, S, dev):
        self.S, self.B, self.h = S, 1, _lib.handle(0)
        lib, B = _lib.lib, 1
        r = ru.NrWrapper(image_size=S).front_renderer
        pts, col, rad = (torch.from_numpy(a).to(dev) for a in debug_clouds())
        self.ndc = r.transform(pts[None]).contiguous()
        self.rad = world_radius_to_pixels(rad[None], self.ndc[..., 2], float(r.focal_pixels())).contiguous()
        self.rad2 = (2 * self.rad).contiguous()
        self.col = col[None].contiguous()
        self.N = self.ndc.shape[1]
        bv, bf = uv_ellipsoid(center=(0.0, 0.0, 2.2))
        sv, sf = icosphere(3, 0.3, (0.6, 0.0, 2.2))
        verts, faces, texts = ru.mesh_tensors([ru.Mesh(v=bv, f=bf), ru.Mesh(v=sv, f=sf)], ru.SMPL_OBJ_COLOR_LIST, dev)
        faces2 = torch.cat((faces, faces.flip(-1)), 1)
        self.tex = torch.cat((texts, texts.permute(0, 1, 4, 3, 2, 5)), 1).contiguous()
        self.light = face_light(vertices_to_faces(verts, faces2), 0.4, 0.3, [1, 1, 1], [1, 1, 1], [1, 0.5, 1]).contiguous()
        self.tri = vertices_to_faces(r.transform(verts), faces2).contiguous()
        self.F = self.tri.shape[1]
        self.op = torch.full((B, self.F), OPACITY, device=dev)
        self.group = torch.cat((ru.mesh_face_group([ru.Mesh(v=bv, f=bf), ru.Mesh(v=sv, f=sf)], dev),) * 2, 1).contiguous()   # both windings
        self.bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        ws = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)       # noqa: E731
        outs = lambda s: [torch.empty(B, 3, s, s, device=dev), torch.empty(B, s, s, device=dev), torch.empty(B, s, s, device=dev)]  # noqa: E731
        self.ws_scene = ws(lib.chore_scene_workspace_bytes(B, self.F, self.N, S, 2))
        self.ws_render, self.ws_splat = ws(lib.chore_render_workspace_bytes(B, self.F, S, 2)), ws(lib.chore_splat_workspace_bytes(B, self.N, S, 2))
        self.ws_render1 = ws(lib.chore_render_workspace_bytes(B, self.F, 2 * S, 1))
        self.ws_splat1 = ws(lib.chore_splat_workspace_bytes(B, self.N, 2 * S, 1))
        self.out_a, self.out_f, self.out_p, self.out_d = outs(S), outs(S), outs(S), outs(S)
        self.lay_f, self.lay_p = outs(2 * S), outs(2 * S)
        self.out_c = None

    def _render(self, size, ssaa, out, ws):
        _lib.check(_lib.lib.chore_render_fwd(self.h, self.tri.data_ptr(), self.tex.data_ptr(), self.light.data_ptr(), self.B, self.F, 4,
                                             size, ssaa, NEAR, FAR, EPS, self.bg, out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr(), None, ws.data_ptr(), self.stream), self.h, "chore_render_fwd")

    def _splat(self, size, ssaa, rad, out, ws):
        _lib.check(_lib.lib.chore_splat_fwd(self.h, self.ndc.data_ptr(), self.col.data_ptr(), rad.data_ptr(), 0.0, self.B, self.N, size,
                                            ssaa, AMBIENT, NEAR, FAR, self.bg, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                            None, ws.data_ptr(), self.stream), self.h, "chore_splat_fwd")

    def run_a(self, opacity=True):
        o = self.out_a
        _lib.check(_lib.lib.chore_scene_fwd(self.h, self.tri.data_ptr(), self.tex.data_ptr(), self.light.data_ptr(),
                                            self.op.data_ptr() if opacity else None, self.B, self.F, 4, self.ndc.data_ptr(),
                                            self.col.data_ptr(), self.rad.data_ptr(), 0.0, self.N, BIAS, self.S, 2, AMBIENT, NEAR, FAR,
                                            EPS, self.bg, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), None,
                                            self.ws_scene.data_ptr(), self.stream), self.h, "chore_scene_fwd")

    def run_d(self, layers):
        o = self.out_d
        _lib.check(_lib.lib.chore_scene_layers_fwd(self.h, self.tri.data_ptr(), self.tex.data_ptr(), self.light.data_ptr(),
                                                   self.op.data_ptr(), self.B, self.F, 4, self.ndc.data_ptr(), self.col.data_ptr(),
                                                   self.rad.data_ptr(), 0.0, self.N, BIAS, self.S, 2, AMBIENT, NEAR, FAR, EPS, self.bg,
                                                   self.group.data_ptr(), layers, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                   None, self.ws_scene.data_ptr(), self.stream), self.h, "chore_scene_layers_fwd")

    def run_b(self):
        self._render(self.S, 2, self.out_f, self.ws_render)
        self._splat(self.S, 2, self.rad, self.out_p, self.ws_splat)

    def run_c(self):
        self._render(2 * self.S, 1, self.lay_f, self.ws_render1)
        self._splat(2 * self.S, 1, self.rad2, self.lay_p, self.ws_splat1)
        (m, zf, af), (p, zn, ap) = self.lay_f, self.lay_p
        front = (ap > 0) & ((af == 0) | ((zn - BIAS) < zf))
        rgb = torch.where(front[:, None], p, m)
        depth = torch.where(front, zn, zf)
        alpha = torch.maximum(af, ap)
        self.out_c = [F.avg_pool2d(rgb, 2), F.avg_pool2d(depth[:, None], 2)[:, 0], F.avg_pool2d(alpha[:, None], 2)[:, 0]]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 60
    trace = "--trace" in sys.argv
    dev = torch.device("cuda:0")
    for S in ((2048,) if trace else (2048, 512)):
        fr = Frame(S, dev)
        rs = fr.rad[0] * 2
        print("image %d px, 2 x 2 samples: %d triangles, %d points (radius in samples: median %.1f, max %.1f); workspace A %.1f MB, "
              "per-sample layers of C %.1f MB" % (S, fr.F, fr.N, float(rs.median()), float(rs.max()), fr.ws_scene.numel() / 1e6,
                                                  2 * 5 * 4 * (2 * S) ** 2 / 1e6), flush=True)
        if trace:
            for _ in range(10):
                fr.run_a()
            torch.cuda.synchronize()
            return
        for _ in range(5):
            fr.run_a()
            fr.run_b()
            fr.run_c()
            for k in (2, 4, 8):
                fr.run_d(k)
        torch.cuda.synchronize()
        ta, tb, tc, td = [], [], [], {2: [], 4: [], 8: []}
        for _ in range(calls):
            ta.append(timed(fr.run_a))
            tb.append(timed(fr.run_b))
            tc.append(timed(fr.run_c))
            for k in td:
                td[k].append(timed(lambda: fr.run_d(k)))
        fr.run_a()
        fr.run_d(1)
        torch.cuda.synchronize()
        one_layer = [bool(torch.equal(a, d)) for a, d in zip(fr.out_a, fr.out_d)]
        fr.run_d(8)
        torch.cuda.synchronize()
        seen = float((fr.out_a[0] != fr.out_d[0]).any(dim=1).float().mean())
        fr.run_a(opacity=False)          # opaque faces: what C composes
        torch.cuda.synchronize()
        same = [bool(torch.equal(a, c)) for a, c in zip(fr.out_a, fr.out_c)]
        print("covered share of the frame: scene %.4f, meshes %.4f, splats %.4f; A with opaque faces equals C bit for bit (rgb, depth, "
              "alpha): %s" % (float((fr.out_a[2] > 0).float().mean()), float((fr.out_f[2] > 0).float().mean()),
                              float((fr.out_p[2] > 0).float().mean()), same))
        print("A  chore_scene_fwd %4d px, 2x:                                    " % S + stats(ta))
        print("B  chore_render_fwd + chore_splat_fwd %4d px, 2x, not composed:   " % S + stats(tb))
        print("C  both at %4d px, 1x, torch select + avg_pool2d:                 " % (2 * S) + stats(tc))
        for k in td:
            print("D  chore_scene_layers_fwd %4d px, 2x, group = mesh, K = %d:         " % (S, k) + stats(td[k]) +
                  "  D / A = %.3f" % (np.median(td[k]) / np.median(ta)))
        print("D with K = 1 equals A bit for bit (rgb, depth, alpha): %s; share of the frame's pixels that K = 8 changes: %.4f"
              % (one_layer, seen))
        spread_b = float(np.percentile(tb, 90) - np.percentile(tb, 10))
        print("median A - median B = %+.3f ms; B's own p10..p90 spread %.3f ms" % (np.median(ta) - np.median(tb), spread_b), flush=True)


if __name__ == "__main__":
    main()
