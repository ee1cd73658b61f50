"""times the photo-texture kernel at the fit's size: a body-sized ellipsoid (13 776 faces) and an object-sized one (2 500 faces)
at 2.2 m through the network's camera, texture cubes of 4^3 texels, visibility on the 512-px grid, a 512 x 512 photo, B = 1 and 8.
Each side is captured into a graph once; windows of 20 replays alternate in one process, device events, per-replay times:
  A  chore_photo_textures_fwd (textures + texel_visible)
  B  a torch composition of the same rule: the texel positions, a gather of the depth image, grid_sample of the photo, where
and reports how far the two sides agree (they round differently, so a texel on a sample boundary may fall either way).
The depth image is made once, outside the timed part, by `sample_depth` for both sides.
    python scripts/photo_textures_bench.py [replays]"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from chore_amd import _lib  # noqa: E402
from chore_amd import render as nr  # noqa: E402
from chore_amd.model.camera import KinectColorCamera  # noqa: E402
from chore_amd.utils import render_utils as ru  # noqa: E402
from chore_amd.utils.synth import uv_ellipsoid  # noqa: E402

NEAR, FAR, BIAS, TS, S, P = 0.1, 100.0, 0.02, 4, 512, 512


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.4f ms  (p10 %.4f, p90 %.4f, min %.4f, max %.4f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def texel_weights(ts, dev):
    i = torch.arange(ts, device=dev, dtype=torch.float32)
    ijk = torch.stack(torch.meshgrid(i, i, i, indexing="ij"), -1)
    w = ijk / ijk.sum(-1, keepdim=True).clamp(min=1)
    w[0, 0, 0] = 1.0 / 3.0
    return w.reshape(-1, 3)                                                   # (ts^3, 3)


def compose(tri, depth, photo, fallback, w):
    """the rule of chore_photo_textures_fwd (align_corners = 1) as torch expressions -> textures (B,F,ts^3,3), visible (B,F,ts^3)"""
    B, Fn = tri.shape[:2]
    zk = tri[..., 2]                                                          # (B,F,3)
    z = (w[None, None] * zk[:, :, None]).sum(-1)                              # (B,F,T)
    s = w[None, None] * zk[:, :, None] / z[..., None]
    u, v = (s * tri[:, :, None, :, 0]).sum(-1), (s * tri[:, :, None, :, 1]).sum(-1)
    xi, yi = torch.floor(0.5 * (u * S + S - 1) + 0.5), torch.floor(0.5 * (v * S + S - 1) + 0.5)
    ok = (NEAR < z) & (z < FAR) & (xi >= 0) & (xi <= S - 1) & (yi >= 0) & (yi <= S - 1)
    idx = (torch.nan_to_num(yi).clamp(0, S - 1) * S + torch.nan_to_num(xi).clamp(0, S - 1)).long().reshape(B, -1)      # NaN: a degenerate face
    d = torch.gather(depth.reshape(B, -1), 1, idx).reshape(z.shape)
    vis = ok & (z <= d + BIAS)
    qx, qy = (u + 1) * 0.5 * (P - 1), (1 - v) * 0.5 * (P - 1)
    inside = (qx >= -0.5) & (qx <= P - 0.5) & (qy >= -0.5) & (qy <= P - 0.5)
    colour = F.grid_sample(photo, torch.stack((u, -v), -1), mode="bilinear", padding_mode="border", align_corners=True)    # (B,3,F,T)
    return torch.where((vis & inside)[..., None], colour.permute(0, 2, 3, 1), fallback[:, :, None, :]), vis


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = fn()
    return g, out


INNER = 20         # replays per timed window: one replay is tens of microseconds


def timed(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER


def main():
    replays = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 60
    dev = torch.device("cuda", 0)
    bv, bf = uv_ellipsoid(center=(0.0, 0.0, 2.2))
    ov, of = uv_ellipsoid(rings=25, segments=50, radii=(0.3, 0.3, 0.3), center=(0.3, 0.1, 1.9))
    verts, faces = ru.mesh_geometry([ru.Mesh(v=bv, f=bf), ru.Mesh(v=ov, f=of)], dev)
    cam = KinectColorCamera()
    cc = torch.tensor([cam.cx_px, cam.cy_px], dtype=torch.float32, device=dev)
    h = _lib.handle(0)
    for B in (1, 8):
        shift = torch.linspace(-0.2, 0.2, B, device=dev).view(B, 1, 1) * torch.tensor([1.0, 0.0, 0.0], device=dev) if B > 1 else 0.0
        ndc = torch.cat([ru._input_view_ndc(cam, v, cc) for v in (verts + shift).expand(B, -1, -1)])
        fc = faces.expand(B, -1, -1)
        tri = nr.vertices_to_faces(ndc, fc).contiguous()
        depth = nr.sample_depth(nr.vertices_to_faces(ndc, torch.cat((fc, fc.flip(-1)), 1)), S, NEAR, FAR)
        Fn = tri.shape[1]
        g = torch.Generator(device=dev).manual_seed(B)
        photo = torch.rand(B, 3, P, P, device=dev, generator=g)
        fallback = torch.rand(B, Fn, 3, device=dev, generator=g)
        w = texel_weights(TS, dev)
        tex = torch.empty(B, Fn, TS, TS, TS, 3, device=dev)
        vis = torch.empty(B, Fn, TS, TS, TS, dtype=torch.uint8, device=dev)

        def run_a():
            _lib.check(_lib.lib.chore_photo_textures_fwd(h, tri.data_ptr(), depth.data_ptr(), photo.data_ptr(), fallback.data_ptr(), B, Fn,
                                                         TS, S, P, P, NEAR, FAR, BIAS, 1, tex.data_ptr(), vis.data_ptr(),
                                                         torch.cuda.current_stream().cuda_stream), h, "A")

        ga, _ = capture(run_a)
        gb, (tex_b, vis_b) = capture(lambda: compose(tri, depth, photo, fallback, w))
        for _ in range(10):
            ga.replay()
            gb.replay()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(replays):
            ta.append(timed(ga))
            tb.append(timed(gb))
        va, vb = vis.bool().reshape(B, Fn, -1), vis_b
        agree = va == vb
        diff = (tex.reshape(B, Fn, -1, 3) - tex_b).abs().amax(-1)[agree].max().item()
        nbytes = tex.numel() * 4 + vis.numel()
        print("B = %d, %d faces, ts %d, S %d, photo %d^2: %.1f %% of the texels visible; the sides disagree on %d of %d texels, "
              "colours differ by at most %.2e elsewhere" % (B, Fn, TS, S, P, 100 * va.float().mean().item(), int((~agree).sum()),
                                                            agree.numel(), diff), flush=True)
        print("  A  chore_photo_textures_fwd:                  " + stats(ta))
        print("  B  torch: gather + grid_sample + where:       " + stats(tb))
        print("  A writes %.2f MB: %.1f GB/s;  median B / median A = %.2f" % (nbytes / 1e6, nbytes / np.median(ta) / 1e6,
                                                                             np.median(tb) / np.median(ta)), flush=True)
        if np.median(ta) > np.median(tb):
            raise SystemExit("the kernel is slower than the torch composition")


if __name__ == "__main__":
    main()
