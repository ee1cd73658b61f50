"""times the training image preparation (TrainImagePrep, csrc/image_prep.hip) on B = 4 Kinect-size frames (1536 x 2048) at
aug_blur 0.01 and 0.05, device events, alternating in one process:
  P  prepare() end to end from images already on the device (draws, 4 masks2bbox calls with their host reads, parameter
     upload, blur, compose)
  B  the blur alone (chore_prep_blur_u8: rows launch + columns launch), buffers preallocated
  C  the compose alone (chore_prep_train_compose), buffers preallocated
and the same batch on the host as the baseline: PIL's GaussianBlur per image (what the reference's loader runs), plus
the numpy restatement of the crop / resize / compose (tests/train_image_ref.py) -- wall clock, a few calls.
Bytes: the blur reads and writes the image twice (the intermediate lives in a workspace), the compose reads at most the
crop windows and writes (B,5,S,S) fp32; against the HBM rate a float4 copy reaches (MI355X: 6.29 TB/s).
    python scripts/train_image_bench.py [calls]"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from chore_amd.data import TrainImagePrep  # noqa: E402

HBM_COPY_RATE = 6.29e12          # bytes / s, float4 copy


def stats(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f ms  (p10 %.3f, p90 %.3f, min %.3f, max %.3f, n = %d)" % (np.median(a), a[len(a) // 10], a[-1 - len(a) // 10],
                                                                               a[0], a[-1], len(a))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def scene(B, H, W, seed):
    rs = np.random.RandomState(seed)
    rgb = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    pm, om = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
    for b in range(B):
        x, y = 500 + 150 * b, 250 + 60 * b
        pm[b, y:y + 900, x:x + 300] = 255
        om[b, y + 400:y + 700, x + 250:x + 600] = 255
    return rgb, pm, om


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 50
    B, H, W, S, crop = 4, 1536, 2048, 512, 1200
    rgb, pm, om = scene(B, H, W, 0)
    d_rgb, d_pm, d_om = (torch.from_numpy(a).cuda() for a in (rgb, pm, om))
    print("B = %d frames of %d x %d, crop %d -> %d, %s" % (B, H, W, crop, S, torch.cuda.get_device_name(0)))
    for aug in (0.01, 0.05):
        prep = TrainImagePrep(image_size=(S, S), crop_size=crop, random_flip=True, aug_blur=aug, seed=1)
        flips, radii = prep.draw(B)
        radii[0] = aug * 255.                                         # the largest radius the setting can draw is in the batch
        prm_h, max_r = prep._params(radii)
        prm = torch.from_numpy(prm_h).cuda()
        centers = np.stack([prep.get_crop_center(d_pm[b], d_om[b]) for b in range(B)])
        tlbr = prep.crop_corners(centers)
        ws, blurred = prep.blur_workspace(d_rgb.shape), torch.empty_like(d_rgb)
        images = torch.empty(B, 5, S, S, dtype=torch.float32, device="cuda")
        run_p = lambda: prep.prepare(d_rgb, d_pm, d_om, flip=flips, blur_radius=radii)           # noqa: E731
        run_b = lambda: prep.blur(d_rgb, prm, max_r, out=blurred, workspace=ws)                   # noqa: E731
        run_c = lambda: prep.compose(blurred, d_pm, d_om, tlbr, flips, out=images)                # noqa: E731
        for _ in range(3):
            run_p(), run_b(), run_c()
        assert torch.equal(run_p()["images"], images)
        torch.cuda.synchronize()
        tp, tb, tc = [], [], []
        for _ in range(calls):
            tp.append(timed(run_p))
            tb.append(timed(run_b))
            tc.append(timed(run_c))
        blur_bytes = 4 * rgb.size                                      # rows: read + write, columns: read + write
        comp_bytes = B * (crop * crop * 5 + 5 * S * S * 4)             # crop windows of rgb + 2 masks (upper bound), fp32 out
        print("aug_blur %.2f: radii %s -> box radius R %s, flips %s" % (aug, np.round(radii, 2).tolist(), prm_h[:, 0].tolist(),
                                                                        flips.astype(int).tolist()))
        print("  P  prepare:        " + stats(tp))
        print("  B  blur alone:     " + stats(tb))
        mb = np.median(tb) * 1e-3
        print("     %.1f MB moved -> %.2f TB/s = %.1f %% of the %.2f TB/s copy rate; HBM lower bound %.3f ms"
              % (blur_bytes / 1e6, blur_bytes / mb / 1e12, 100 * blur_bytes / mb / HBM_COPY_RATE, HBM_COPY_RATE / 1e12,
                 blur_bytes / HBM_COPY_RATE * 1e3))
        print("  C  compose alone:  " + stats(tc))
        mc = np.median(tc) * 1e-3
        print("     <= %.1f MB moved -> %.2f TB/s; HBM lower bound %.3f ms" % (comp_bytes / 1e6, comp_bytes / mc / 1e12,
                                                                                comp_bytes / HBM_COPY_RATE * 1e3))
        # the host baseline
        try:
            from PIL import Image
            from PIL.ImageFilter import GaussianBlur
        except ImportError:
            print("  host baseline: PIL is not installed, not measured")
            continue
        from train_image_ref import train_crop_ref
        th_blur, th_all = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            host_blurred = [np.array(Image.fromarray(np.ascontiguousarray(rgb[b][:, ::-1] if flips[b] else rgb[b])).filter(GaussianBlur(radii[b])))
                            for b in range(B)]
            t1 = time.perf_counter()
            # train_crop_ref with radius 0 on the blurred, already mirrored RGB: the masks are mirrored here
            ref = [train_crop_ref(host_blurred[b], pm[b][:, ::-1] if flips[b] else pm[b], om[b][:, ::-1] if flips[b] else om[b],
                                  centers[b], False, 0.0, (S, S), crop) for b in range(B)]
            th_blur.append((t1 - t0) * 1e3)
            th_all.append((time.perf_counter() - t0) * 1e3)
        print("  host: PIL blur of the batch " + stats(th_blur))
        print("  host: PIL blur + numpy crop / resize / compose " + stats(th_all) + "   P is %.0f x faster" % (np.median(th_all) / np.median(tp)))
        print("  host result equals the device's: %s" % np.array_equal(np.stack(ref), images.cpu().numpy()))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
