"""one inference encoder pass and one training step at bench.py's shapes (4 images of 512 x 512, 20 000 points each) in one precision
mode, everything on one stream (CHORE_ENC_SERIAL, CHORE_CONVBLOCK_SERIAL) so that a kernel trace lists the launches in the order
they were issued.  Run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/conv_plan_trace.py MODE`, once
per mode (fp16x3, bf16, fp32, fp16; fp16 maps are an inference mode: no training step there): the ordered `conv_*_kernel` names of
two commits must agree line by line (profiles/conv_plan_trace.txt).  Between the two it runs the encoder once more with the
library's profile on and prints the launches per profile class, which must name the kernels of the trace.
`--names FILE.csv` prints the ordered convolution kernels of a trace; `--layers MODE` (no profiler needed) prints the encoder's
convolution steps in issue order (the step labels of CHORE_DEBUG_SYNC), one per kernel of the trace's first pass."""
import csv
import os
import re
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
CONV = re.compile(r"^conv_(lds|small|pc|mw|rw)_kernel")


def names(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ks = [r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0] for r in rows]
    return [k for k in ks if CONV.match(k)]


def main(mode, train=True):
    os.environ.update(CHORE_ENC_SERIAL="1", CHORE_CONVBLOCK_SERIAL="1")
    import numpy as np
    import torch
    import bench
    from chore_amd import _lib
    from chore_amd.model import CHORE
    from chore_amd.utils import synth
    dev = torch.device("cuda", 0)
    B, N = 4, 20000
    net = CHORE(bench.chore_opt(mode)).to(dev).eval()
    synth.load_synth_weights(net, seed=0)
    images = torch.from_numpy(synth.synth_images(B, 512, 512, seed=0)).to(dev)
    with torch.no_grad():
        net.filter(images)
        torch.cuda.synchronize()
        print("inference pass done", flush=True)
        if not train:
            return
        _lib.profile_enable(0, True)
        net.filter(images)
        prof = _lib.profile_read(0)
        _lib.profile_enable(0, False)
    for k, v in prof.items():
        if v["launches"] and k.startswith("conv_"):
            print("class %-34s %3d launches" % (k, v["launches"]), flush=True)
    if mode == "fp16":
        return
    net.train(True)
    net.losses_on_host = False
    rs = np.random.RandomState(50)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    batch = dict(images=images, points=t(synth.synth_points(B, N, seed=1)),
                 df_h=t(rs.uniform(0, 0.3, (B, N)).astype(np.float32)), df_o=t(rs.uniform(0, 0.3, (B, N)).astype(np.float32)),
                 parts_gt=t(rs.randint(0, 14, (B, N))), pca_gt=t(rs.standard_normal((B, 3, 3, N)).astype(np.float32)),
                 body_center=t((rs.standard_normal((B, 3)) * 0.3).astype(np.float32)),
                 obj_center=t((rs.standard_normal((B, 3, N)) * 0.3).astype(np.float32)),
                 crop_center=torch.tensor([synth.CROP_CENTER] * B, dtype=torch.float32, device=dev))
    error, _ = net(**batch)
    error.backward()
    torch.cuda.synchronize()
    print("training step done, loss %.6g" % float(error), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--names"]:
        print("\n".join(names(sys.argv[2])))
    elif sys.argv[1:2] == ["--layers"]:     # a child with CHORE_DEBUG_SYNC: the library prints every step's label
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--inference-only", sys.argv[2]], capture_output=True, text=True,
                           env=dict(os.environ, CHORE_DEBUG_SYNC="1"))
        if r.returncode:
            sys.exit(r.stderr[-2000:])
        print("\n".join(l[len("[chore] step "):] for l in r.stderr.splitlines() if l.startswith("[chore] step conv ")))
    elif sys.argv[1:2] == ["--inference-only"]:
        main(sys.argv[2], train=False)
    else:
        main(sys.argv[1])
