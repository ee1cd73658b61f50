"""every call of tests/query_plan_cases.py once, in the list's order, on one stream: prints one sha256 per call over all of the
call's outputs.  Run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/query_plan_trace.py`, once per
switch set of the case file (the switches are read once per process, so each set is a process of its own): the ordered `query_*`
kernel names of the trace are what the case file's expectations are written from, and the digests of two commits must agree line
by line.  `--names FILE.csv` prints that ordered list from a trace instead, one line per call ("sort + " where the sort ran first).
Random maps of 16 x 16 (feat) and 32 x 32 (tmpx) texels, except where a case names the feature map's size."""
import csv
import ctypes
import hashlib
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tests")]
import query_plan_cases as qc  # noqa: E402


def names(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ks = [r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0] for r in rows]
    out, sort = [], ""
    for k in ks:
        if k.startswith(("query_bin_kernel", "query_perm_kernel")):
            sort = "sort + "
        elif k.startswith("query_"):
            out.append(sort + k)
            sort = ""
    return out


def main():
    import torch
    from chore_amd import _lib
    from chore_amd.model.camera import KinectColorCamera
    from chore_amd.utils import synth
    L, dev = _lib.lib, torch.device("cuda", 0)
    h = _lib.handle(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device="cpu").manual_seed(7)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    named = []
    for hd, odim in (("df", 2), ("part_predictor", 14), ("pca_predictor", 9), ("center_predictor", 6)):
        for l, (i, o) in enumerate(((323, 128), (128, 128), (128, 128), (128, odim))):
            named += [("%s.%d.weight" % (hd, 2 * l), rnd(o, i, scale=i ** -0.5)), ("%s.%d.bias" % (hd, 2 * l), rnd(o, scale=0.1))]
    arena = torch.empty(L.chore_heads_arena_bytes(_lib.F32), dtype=torch.uint8, device=dev)
    descs, keep = _lib.make_descs(named)
    _lib.check(L.chore_heads_pack(h, descs, len(named), _lib.F32, arena.data_ptr(), stream), h, "chore_heads_pack")
    cam6 = (ctypes.c_float * 6)(*KinectColorCamera().kernel_constants())
    tdt = {qc.F32: torch.float32, qc.BF16: torch.bfloat16, qc.F16: torch.float16}
    maps, points, staging = {}, {}, {}
    for i, (op, dtype, B, N, FH, FW, live, flags, _) in enumerate(qc.CASES):
        mt = qc.F32 if dtype == qc.F16X3 else dtype & ~qc.X3
        if (mt, FH, FW) not in maps:       # NHWC, batch of 4: a case reads the first B images
            maps[mt, FH, FW] = (rnd(4, FH, FW, 256).to(tdt[mt]), rnd(4, 32, 32, 64).to(tdt[mt]))
        feat, tmpx = maps[mt, FH, FW]
        if (B, N) not in points:
            points[B, N] = (torch.from_numpy(synth.synth_points(B, N, seed=3)).to(dev), torch.tensor([synth.CROP_CENTER] * B, device=dev))
        pts, cc = points[B, N]
        head = (h, pts.data_ptr(), cc.data_ptr(), B, N, feat.data_ptr(), FH, FW, tmpx.data_ptr(), 32, 32, dtype, arena.data_ptr(), cam6)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        outs = [z(B, 2, N), z(B, 9, N), z(B, 14, N), z(B, 6, N)]            # df, pca, parts, centers (the entry points' order)
        grads = [rnd(B, c, N) if live >> bit & 1 else None for c, bit in ((2, 0), (9, 2), (14, 1), (6, 3))]
        gp = [None if t is None else t.data_ptr() for t in grads]
        if op in (qc.FWD_TRAIN, qc.BWD_TRAIN) and (B, N) not in staging:
            staging[B, N] = z(L.chore_query_train_bytes(B, N), dt=torch.uint8)
        if op == qc.FWD:
            ws = z(L.chore_query_fwd_workspace_bytes(B, N), dt=torch.uint8) if flags & qc.WS else None
            rc = L.chore_query_fwd_ws(*head, *[t.data_ptr() for t in outs], None, None if ws is None else ws.data_ptr(), stream)
        elif op == qc.FWD_TRAIN:
            outs += [z(B, N, dt=torch.uint8), staging[B, N]]
            rc = L.chore_query_fwd_train(*head, *[t.data_ptr() for t in outs], stream)
        elif op == qc.BWD_POINTS:
            outs = [z(B, N, 3)]
            rc = L.chore_query_bwd_points(*head, *gp, outs[0].data_ptr(), stream)
        elif op == qc.SURFACE_STEP:
            outs = [z(B, N, 3)]
            rc = L.chore_gen_surface_step_fused(*head, i & 1, 0.3, outs[0].data_ptr(), stream)
        else:
            outs = [z(B, N, 3), staging[B, N]]
            rc = L.chore_query_bwd_train(*head, *gp, staging[B, N].data_ptr(), outs[0].data_ptr(), 1 if flags & qc.HF else 0, stream)
        _lib.check(rc, h, "case %d" % i)
        torch.cuda.synchronize()
        d = hashlib.sha256()
        for t in outs:
            d.update(t.cpu().numpy().tobytes())
        print("%3d %s" % (i, d.hexdigest()), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--names"]:
        print("\n".join(names(sys.argv[2])))
    else:
        main()
