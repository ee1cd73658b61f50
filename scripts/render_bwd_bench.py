"""times the backward of the colour / depth renderer on render_bench.py's demo view (B = 1, a body-sized ellipsoid at 2.2 m and
a sphere of radius 0.3 beside it: 30 112 triangles after fill_back, ts = 4) at 2048 px and at 256 px, 2x super-sampling.
Alternating in one process, device events:
  F   chore_render_fwd with sample_face_index (what the differentiable forward runs)
  FB  the same call followed by chore_render_bwd with all three upstream gradients, grad_textures and grad_light
and FB - F = the backward alone.  Also prints the workspace bytes of both calls and how unevenly the samples are owned (the
gather kernel gives a triangle to one workgroup).
    python scripts/render_bwd_bench.py [calls] [--trace]
--trace: a few FB calls at each size and nothing else, for `rocprofv3 --kernel-trace --stats` (the share of each launch)"""
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
from chore_amd.render import face_light  # noqa: E402
from chore_amd.utils import render_utils as ru  # noqa: E402
from chore_amd.utils.synth import uv_ellipsoid  # noqa: E402
from meshes import icosphere  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f ms  (p10 %.3f, p90 %.3f, min %.3f, max %.3f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def view(size, dev):
    """the demo view at `size` px: everything both calls need, and the two closures"""
    h = _lib.handle(0)
    bv, bf = uv_ellipsoid(center=(0.0, 0.0, 2.2))
    sv, sf = icosphere(3, 0.3, (0.6, 0.0, 2.2))
    nrw = ru.NrWrapper(image_size=size)
    r = nrw.front_renderer
    verts, faces, texts = nrw.prepare_render([ru.Mesh(v=bv, f=bf), ru.Mesh(v=sv, f=sf)])
    faces2 = torch.cat((faces, faces.flip(-1)), 1)
    tex = torch.cat((texts, texts.permute(0, 1, 4, 3, 2, 5)), 1).contiguous()
    light = face_light(vertices_to_faces(verts, faces2), 0.4, 0.3, [1, 1, 1], [1, 1, 1], [1, 0.5, 1]).contiguous()
    tri = vertices_to_faces(r.transform(verts), faces2).contiguous()
    B, Fn, ts, ssaa = tri.shape[0], tri.shape[1], tex.shape[2], 2
    nf, nb = _lib.lib.chore_render_workspace_bytes(B, Fn, size, ssaa), _lib.lib.chore_render_bwd_workspace_bytes(B, Fn, ts, size, ssaa)
    ws_f, ws_b = torch.empty(nf, dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)
    rgb = torch.empty(B, 3, size, size, device=dev)
    depth, alpha = torch.empty(B, size, size, device=dev), torch.empty(B, size, size, device=dev)
    fim = torch.empty(B, size * ssaa, size * ssaa, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    g_rgb = torch.randn(rgb.shape, device=dev, generator=gen)
    g_depth, g_alpha = torch.randn(depth.shape, device=dev, generator=gen), torch.randn(depth.shape, device=dev, generator=gen)
    g_tri, g_tex, g_light = torch.empty_like(tri), torch.empty_like(tex), torch.empty_like(light)
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fwd():
        _lib.check(_lib.lib.chore_render_fwd(h, tri.data_ptr(), tex.data_ptr(), light.data_ptr(), B, Fn, ts, size, ssaa, 0.1, 100.0,
                                             1e-3, bg, rgb.data_ptr(), depth.data_ptr(), alpha.data_ptr(), fim.data_ptr(),
                                             ws_f.data_ptr(), stream), h, "chore_render_fwd")

    def fwd_bwd():
        fwd()
        _lib.check(_lib.lib.chore_render_bwd(h, tri.data_ptr(), tex.data_ptr(), light.data_ptr(), fim.data_ptr(), B, Fn, ts, size,
                                             ssaa, 0.1, 100.0, 1e-3, 1e-3, bg, g_rgb.data_ptr(), g_depth.data_ptr(),
                                             g_alpha.data_ptr(), g_tri.data_ptr(), g_tex.data_ptr(), g_light.data_ptr(),
                                             ws_b.data_ptr(), stream), h, "chore_render_bwd")
    return dict(fwd=fwd, fwd_bwd=fwd_bwd, fim=fim, Fn=Fn, nf=nf, nb=nb, outs=(g_tri, g_tex, g_light))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 40
    trace = "--trace" in sys.argv
    dev = torch.device("cuda:0")
    for size in (2048, 256):
        v = view(size, dev)
        if trace:
            for _ in range(5):
                v["fwd_bwd"]()
            torch.cuda.synchronize()
            continue
        for _ in range(3):
            v["fwd"]()
            v["fwd_bwd"]()
        torch.cuda.synchronize()
        tf, tfb = [], []
        for _ in range(calls):
            tf.append(timed(v["fwd"]))
            tfb.append(timed(v["fwd_bwd"]))
        fim = v["fim"]
        own = torch.bincount(fim[fim >= 0].long(), minlength=v["Fn"]).float()
        top = torch.sort(own, descending=True).values
        print("== %d px, 2x: %d triangles, workspace forward %.1f MB, backward %.1f MB" % (size, v["Fn"], v["nf"] / 2 ** 20, v["nb"] / 2 ** 20))
        print("F   forward with sample_face_index:   " + stats(tf))
        print("FB  forward + backward:               " + stats(tfb))
        print("FB - F (medians), the backward alone: %.3f ms = %.2f x the forward" % (np.median(tfb) - np.median(tf),
                                                                                  (np.median(tfb) - np.median(tf)) / np.median(tf)))
        print("samples owned: covered %.4f of the grid, %d triangles own one or more, the largest owner %d samples, "
              "the 1 %% largest owners %.3f of the covered samples" % (float((fim >= 0).float().mean()), int((own > 0).sum()), int(top[0]),
                                                                      float(top[:max(1, v["Fn"] // 100)].sum() / own.sum())))
        print("gradients: |grad_tri| max %.4g, |grad_textures| max %.4g, |grad_light| max %.4g, all finite: %s"
              % (v["outs"][0].abs().max().item(), v["outs"][1].abs().max().item(), v["outs"][2].abs().max().item(),
                 all(bool(torch.isfinite(o).all()) for o in v["outs"])), flush=True)
        del v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
