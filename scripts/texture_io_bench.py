"""times the two kernels of the textured-OBJ interface at SMPL size (13 776 faces) and at a 100 000-face scan, texture cubes of
4^3 texels:
  load   chore_load_textures: UV triangles scattered over one 2048 x 2048 RGB image, REPEAT, bilinear
  atlas  chore_texture_atlas: the cubes into tiles of 16 px (1872 x 1888 px for the body, 5056 x 5072 px for the scan)
each against a torch composition of the same rule (the same fp32 operations in the same order: fmod / where for the wrap, eight
or four gathers, lerps), which is first checked against the kernel.  Each side is captured into a graph once; windows of 20
replays alternate in one process, device events, per-replay times.  Nothing here is a condition: the script reports.
    python scripts/texture_io_bench.py [windows]"""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from chore_amd import _lib  # noqa: E402
from chore_amd.render import obj_io  # noqa: E402

TS, TSO, IMG = 4, 16, 2048
SIZES = (("SMPL", 13776), ("scan", 100000))
INNER = 20         # replays per timed window


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.4f ms  (p10 %.4f, p90 %.4f, min %.4f, max %.4f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def texel_weights(ts, dev):
    i = torch.arange(ts, device=dev, dtype=torch.float32) / float(ts - 1)
    d = torch.stack(torch.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    s = (d[:, 0] + d[:, 1]) + d[:, 2]
    return torch.where(s[:, None] > 0, d / torch.where(s > 0, s, torch.ones_like(s))[:, None], d)        # (ts^3, 3)


def compose_load(uv, face_image, face_color, image, d):
    """chore_load_textures (REPEAT, bilinear, one image) as torch expressions -> (F, ts^3, 3)"""
    H, W = image.shape[:2]
    r = torch.fmod(uv, 1.0)
    w = torch.where(uv > 0, r, 1.0 + r)                                                                  # (F,3,2)
    pos = (w[:, None, 0, :] * d[None, :, 0, None] + w[:, None, 1, :] * d[None, :, 1, None]) + w[:, None, 2, :] * d[None, :, 2, None]
    px, py = pos[..., 0] * float(W - 1), pos[..., 1] * float(H - 1)                                      # (F,T)
    xi, yi = px.to(torch.int32), py.to(torch.int32)
    fx, fy = (px - xi)[..., None], (py - yi)[..., None]
    x0, y0 = xi.clamp(0, W - 1).long(), yi.clamp(0, H - 1).long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    tap = lambda y, x: image[H - 1 - y, x].float() / 255.0                                               # noqa: E731
    a, b = tap(y0, x0), tap(y1, x0)
    top = a + (tap(y0, x1) - a) * fx
    bot = b + (tap(y1, x1) - b) * fx
    return torch.where((face_image >= 0)[:, None, None], top + (bot - top) * fy, face_color[:, None, :])


def compose_atlas(tex, tso):
    """chore_texture_atlas as torch expressions -> (H, W, 3)"""
    Fn, tsi = tex.shape[:2]
    dev = tex.device
    hh, ww = obj_io.atlas_size(Fn, tso)
    tile_w, T, eps = ww // tso, tso - 1, 1e-5
    y = (hh - 1 - torch.arange(hh, device=dev))[:, None].expand(hh, ww)
    x = torch.arange(ww, device=dev)[None, :].expand(hh, ww)
    fn = x // tso + (y // tso) * tile_w
    lx, ly = x % tso, y % tso
    lx = lx - (ly + 1 == lx).long()
    den = 1.0 + eps
    w = torch.stack([((T - ly).float() / T) / den, ((ly - lx).float() / T) / den, (lx.float() / T) / den], -1)
    t = (w * float(tsi - 1)).clamp(min=0.0).clamp(max=float(tsi - 1) - eps)
    lo = t.to(torch.int32).long().clamp(0, tsi - 1)
    hi = (lo + 1).clamp(max=tsi - 1)
    fr = t - lo
    flat = tex.reshape(Fn, tsi ** 3, 3)
    face = fn.clamp(max=Fn - 1)
    texel = lambda a, b, c: flat[face, (a * tsi + b) * tsi + c]                                          # noqa: E731
    planes = []
    for a in (lo[..., 0], hi[..., 0]):
        lines = []
        for b in (lo[..., 1], hi[..., 1]):
            v0 = texel(a, b, lo[..., 2])
            lines.append(v0 + (texel(a, b, hi[..., 2]) - v0) * fr[..., 2:3])
        planes.append(lines[0] + (lines[1] - lines[0]) * fr[..., 1:2])
    out = planes[0] + (planes[1] - planes[0]) * fr[..., 0:1]
    return torch.where((fn < Fn)[..., None], out, torch.zeros_like(out))


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


def timed(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER


def compare(name, ga, gb, out_a, out_b, windows, nbytes, tol):
    for _ in range(5):
        ga.replay()
        gb.replay()
    torch.cuda.synchronize()
    diff = (out_a.reshape(out_b.shape) - out_b).abs().max().item()
    if not diff <= tol:
        raise SystemExit("%s: the torch composition and the kernel differ by %g" % (name, diff))
    ta, tb = [], []
    for _ in range(windows):
        ta.append(timed(ga))
        tb.append(timed(gb))
    print("  A  %-24s " % name + stats(ta))
    print("  B  torch composition:       " + stats(tb))
    print("  the two differ by at most %.2e;  A reads and writes %.2f MB: %.1f GB/s;  median B / median A = %.2f"
          % (diff, nbytes / 1e6, nbytes / np.median(ta) / 1e6, np.median(tb) / np.median(ta)), flush=True)


def main():
    windows = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 60
    dev = torch.device("cuda", 0)
    h = _lib.handle(0)
    g = torch.Generator(device=dev).manual_seed(0)
    image = torch.randint(0, 256, (IMG, IMG, 3), device=dev, generator=g, dtype=torch.uint8)
    off_c, hw_c = (ctypes.c_int64 * 1)(0), (ctypes.c_int * 2)(IMG, IMG)
    d = texel_weights(TS, dev)
    for label, Fn in SIZES:
        # triangles of about 1 % of the image, scattered over [-0.5, 1.5]^2 so that the wrap has work; every 16th face colour-only
        uv = (torch.rand(Fn, 1, 2, device=dev, generator=g) * 2 - 0.5 + (torch.rand(Fn, 3, 2, device=dev, generator=g) - 0.5) * 0.02)
        uv = uv.contiguous()
        face_image = torch.where(torch.arange(Fn, device=dev) % 16 == 15, -1, 0).to(torch.int32)
        face_color = torch.rand(Fn, 3, device=dev, generator=g)
        tex = torch.empty(Fn, TS, TS, TS, 3, device=dev)
        hh, ww = obj_io.atlas_size(Fn, TSO)
        atlas = torch.empty(hh, ww, 3, device=dev)

        def run_load():
            _lib.check(_lib.lib.chore_load_textures(h, uv.data_ptr(), face_image.data_ptr(), face_color.data_ptr(), image.data_ptr(),
                                                    image.numel(), off_c, hw_c, 1, Fn, TS, 0, 1, tex.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), h, "chore_load_textures")

        def run_atlas():
            _lib.check(_lib.lib.chore_texture_atlas(h, tex.data_ptr(), Fn, TS, TSO, atlas.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), h, "chore_texture_atlas")

        print("%s: %d faces, ts %d, image %d^2, atlas %d x %d px" % (label, Fn, TS, IMG, hh, ww), flush=True)
        ga, _ = capture(run_load)
        gb, tex_b = capture(lambda: compose_load(uv, face_image, face_color, image, d))
        # bytes: the texels written, the UVs, colours and indices read; the taps read from the image are not counted
        compare("chore_load_textures:", ga, gb, tex, tex_b, windows, tex.numel() * 4 + uv.numel() * 4 + Fn * 16, 1e-3)
        del gb, tex_b
        ga, _ = capture(run_atlas)
        gb, atlas_b = capture(lambda: compose_atlas(tex, TSO))
        compare("chore_texture_atlas:", ga, gb, atlas, atlas_b, windows, atlas.numel() * 4 + tex.numel() * 4, 2e-5)
        del gb, atlas_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
