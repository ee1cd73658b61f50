#!/usr/bin/env python
"""bench.py -- the benchmarks of the CHORE field-query / fitting hot path on MI355X, one JSON line each.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--mode all|query|fit|train] [--full] [--dump-outputs DIR]

A plain run (no --full) of --mode all or --mode query measures the headline only: set up, W warm-up steps, the K timed query
    steps, the outputs if --dump-outputs is given, the line (metric, value, unit, dtype, ms_per_step, ...).  Nothing else runs.
--full: everything else the benchmark measures and checks, after the timed region, as listed below.  --mode fit and
    --mode train print their whole records either way.
--dump-outputs DIR: after the timed steps, rank 0 writes what its last timed query step computed -- df, pca, parts, centers
    of CHORE.get_preds(), float32 -- as DIR/<name>.npy.  The inputs are seeded: the same arguments give the same inputs.

--mode all (default) with --full: the line of --mode query (the K timed steps are query steps) and, measured after
    the timed region by the same functions, the sub-records "fit" (metric 2) and "train" (metric 3), each with its own value,
    roofline and cpu_baseline, plus query_fwd_bwd_points_per_s (metric 1(ii): forward + backward to the points).  With
    N > 1 the "train" record is DDP over RCCL and carries the all-reduce share (a synced step against a no_sync() step);
    the "fit" record is the frame-sharded fit (8 frames per GPU, one gather).

--mode query (default; BASELINE.json metric 1, configs[1]): per GPU ONE STEP = HGFilters encode of 4 synthetic 512x512
    5-channel images + one 20 000-point MLP field query per image = `CHORE.filter(images); CHORE.query(points, crop_center)`
    through libchore_hip.so.  value = query points per second, whole job.  Default precision: fp16x3 (fp32 tensors,
    convolutions on the fp16 matrix cores with hi/lo split operands), the fastest mode whose field values stay within the
    north-star tolerance of 1e-4; the bf16 mode BASELINE names (1e-2 field error) and native fp32 are timed beside it.
--mode fit (metric 2, configs[2]; with N > 1 configs[4]): ONE STEP = the whole fit_recon chain for one batch of frames --
    encode, point-cloud generation, SMPL-H initialisation, optimize_smpl, object initialisation, optimize_smpl_object
    with the silhouette, contact and collision terms -- run with schedules of exactly 100 + 200 = 300 Adam iterations
    (stop rule off), every inner iteration a hipGraph replay.  value = ms per fit iteration.
--mode train (metric 3, configs[3]): ONE STEP = CHORE.forward (5 stacks) + backward + Adam on 4 images x 20 000 points
    per GPU, gradients all-reduced by torch DDP over RCCL when N > 1.  value = training steps per second.

With --gpus N > 1 and no launcher environment the script re-launches itself as
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`
(one process per GPU); the driver's own launch line does the same.  Every mode: W untimed warm-up steps, then exactly K
steps bracketed by barrier + synchronize on both sides, MAX over ranks, rank 0 prints the line.  The work shards by
image / frame: every rank runs the same per-GPU workload on its own seeded inputs ("scaling": "weak"); the
only collectives are the barriers, the MAX-reduce of the time and, in train mode, DDP's gradient all-reduce.

Extra objects in the line (--full):
  roofline            query: the kernel class with the largest measured time per step -- ALGORITHMIC FLOPs per launch /
                      average launch duration measured live with hipEvents on the launch stream (chore_profile_enable;
                      that pass runs the encoder on ONE stream so kernels do not overlap) against the dense MFMA peak of
                      its dtype; kernel names are the rocprofv3 names.  fit / train: the whole step against the same
                      peak (named so in `kernel`).
  config.field_err    query: measured error of df / pca / parts / centers against the values THE REFERENCE produced for the
                      same images and points (tests/golden/config2_fields.npz) in the timed mode; `other_modes` holds the
                      same step in the two fp32-grade modes with their own timing and error: "fp16x3" (fp32 tensors,
                      convolutions as three fp16 MFMAs per product on hi/lo split operands) and "fp32" (native fp32 MFMA).
  cpu_baseline        the numpy oracle ("port") and `cpu_baseline_torch` the same graph as stock PyTorch CPU operators
                      (oracle/torch_graph.py), timed on this host on a bounded sample, rank 0, N = 1 only.
"""
import argparse
import json
import os

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for multi-process RCCL on this driver
import socket
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md.  fp16x3 issues three fp16 MFMAs per algorithmic product: its
# algorithmic FLOPs are priced against the full fp16 peak (a kernel doing nothing but MFMAs would show frac = 1/3)
PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3, "fp16x3": 2500.0, "fp16": 2500.0}
TNAME = {"bf16": "unsigned short", "fp32": "float", "fp16x3": "x3_t", "fp16": "h16_t"}
HEADS_FLOP_PER_POINT = 600832.0
ENCODER_FLOP_PER_IMAGE = 258.25e9            # the reference graph (training: l, bl, al separate), SURVEY 8(d)
# eval merges l / bl / al of stacks 0-3 into one 1x1 convolution (csrc/encoder.hip): 2 x 4 convolutions of
# 2 * 256 * 256 * 128^2 FLOP per image are not executed
ENCODER_FLOP_PER_IMAGE_EVAL = ENCODER_FLOP_PER_IMAGE - 8 * 2.0 * 256 * 256 * 128 * 128


def chore_opt(dtype):
    return argparse.Namespace(input_type="RGBM3", norm="group", num_stack=5, num_hourglass=2, hg_down="ave_pool",
                              hourglass_dim=256, skip_hourglass=True, z_feat="xyz", projection_mode="perspective",
                              loadSize=1200, net_img_size=[512, 512], gpu_id=0, compute_dtype=dtype)


def _spec():
    return [(k, tuple(s)) for k, s in json.load(open(os.path.join(REPO, "tests", "golden", "state_dict_spec.json")))]


def _host_threads():
    try:
        from threadpoolctl import threadpool_info
        return max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
    except Exception:
        return os.cpu_count() or 1


# ---- CPU baselines (rank 0, N = 1 only; bounded samples) ---------------------------------------------------------------
def cpu_baseline_query():
    """numpy oracle on the host cores: 1 image encode + 20 000-point query (a quarter of one step)"""
    from chore_amd.utils import synth
    from oracle import encoder as oe, query as oq
    sd = synth.synth_state_dict(_spec(), seed=0)
    img = synth.synth_images(1, 512, 512, seed=0)
    pts = synth.synth_points(1, 20000, seed=1)
    cc = np.array([synth.CROP_CENTER], np.float32)
    t0 = time.perf_counter()
    outs, tmpx, _ = oe.Encoder(sd).forward(img)
    t1 = time.perf_counter()
    oq.query(pts, cc, outs[-1], tmpx, sd)
    t2 = time.perf_counter()
    return {"value": 20000.0 / (t2 - t0), "unit": "points/s", "cores": int(_host_threads()), "kind": "port",
            "sample": "numpy oracle: 1 image 512x512 encode (%.2f s) + 20000-point query (%.3f s) = 1/4 step"
                      % (t1 - t0, t2 - t1),
            "host_cpus": os.cpu_count()}


def cpu_baseline_query_torch(reps=3):
    """the same graph as stock PyTorch CPU operators (what the reference executes): 1 image + 20 000 points, best of reps"""
    from chore_amd.utils import synth
    from oracle import torch_graph as tg
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(_spec(), seed=0).items()}
    img = torch.from_numpy(synth.synth_images(1, 512, 512, seed=0))
    pts = torch.from_numpy(synth.synth_points(1, 20000, seed=1))
    cc = torch.tensor([synth.CROP_CENTER])
    best = None
    with torch.no_grad():
        for _ in range(reps + 1):          # first pass warms the thread pool / allocator
            t0 = time.perf_counter()
            outs, tmpx, _ = tg.encoder(img, sd)
            t1 = time.perf_counter()
            tg.query(pts, cc, outs[-1], tmpx, sd)
            t2 = time.perf_counter()
            if best is None or t2 - t0 < best[0]:
                best = (t2 - t0, t1 - t0, t2 - t1)
    return {"value": 20000.0 / best[0], "unit": "points/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": "stock torch CPU ops of the same graph (oracle/torch_graph.py): 1 image 512x512 encode (%.3f s) + "
                      "20000-point query (%.3f s) = 1/4 step, best of %d" % (best[1], best[2], reps)}


def cpu_baseline_fit(reps=3):
    """the field part of ONE fit iteration as stock torch CPU ops: forward + backward-to-points of the 6 890 SMPL vertices
    and twice the 3 000 object points (recon_fit_behave.py:179,196,204) on one image's maps -- a lower bound of the
    reference's CPU time per iteration (LBS, priors, contact and Adam come on top)"""
    from chore_amd.utils import synth
    from oracle import torch_graph as tg
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(_spec(), seed=0).items()}
    rs = np.random.RandomState(3)
    feat = torch.from_numpy(rs.standard_normal((1, 256, 128, 128)).astype(np.float32))
    tmpx = torch.from_numpy(rs.standard_normal((1, 64, 256, 256)).astype(np.float32))
    cc = torch.tensor([synth.CROP_CENTER])
    best = None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        for n in (6890, 3000, 3000):
            p = torch.from_numpy(synth.synth_points(1, n, seed=n)).requires_grad_(True)
            df = tg.query(p, cc, feat, tmpx, sd)[0]
            df.clamp(max=0.8).mean().backward()
        t = time.perf_counter() - t0
        best = t if best is None or t < best else best
    return {"value": best * 1e3, "unit": "ms", "cores": torch.get_num_threads(), "kind": "port",
            "sample": "stock torch CPU ops: field queries of one fit iteration (6890 + 2 x 3000 points, forward + "
                      "backward to the points), 1 frame, best of %d; LBS / priors / contact / Adam not included" % reps}


def cpu_baseline_train():
    """forward + backward of the training loss as stock torch CPU ops on 1 image x 20 000 points (1/4 of a GPU's batch)"""
    from chore_amd.utils import synth
    from oracle import torch_graph as tg
    sd = {k: torch.from_numpy(v).requires_grad_(True) for k, v in synth.synth_state_dict(_spec(), seed=0).items()}
    img = torch.from_numpy(synth.synth_images(1, 512, 512, seed=0))
    pts = torch.from_numpy(synth.synth_points(1, 20000, seed=1))
    cc = torch.tensor([synth.CROP_CENTER])
    t0 = time.perf_counter()
    outs, tmpx, _ = tg.encoder(img, sd)
    loss = 0
    for o in outs:
        df, pca, parts, centers = tg.query(pts, cc, o, tmpx, sd)
        loss = loss + df.clamp(max=5.0).abs().sum(-1).mean() + parts.square().mean() + pca.square().mean() + centers.square().mean()
    loss.backward()
    t = time.perf_counter() - t0
    return {"value": 1.0 / (4 * t), "unit": "steps/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": "stock torch CPU ops: encoder + 5 field queries + a loss of the same shape, forward + backward, 1 image x "
                      "20000 points (%.2f s) = 1/4 of a per-GPU step; no optimiser" % t}


# ---- launch -----------------------------------------------------------------------------------------------------------
def self_launch(n):
    """re-run this script as one process per GPU (the line the driver uses for N > 1)"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    import subprocess
    raise SystemExit(subprocess.call(cmd))        # a child process, not exec: this one has loaded torch


class Ctx:
    """rank / device / collectives of this process"""

    def __init__(self, gpus, backend=None, one_rank_group=False, use_gpu=True):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local = int(os.environ.get("LOCAL_RANK", "0"))
        # Rehearsal of the N > 1 code path on a ONE-GPU box (no multi-GPU box was ever available to the builder): every rank on device 0
        # and gloo moving the device tensors (RCCL refuses two ranks on one device).  Timings of such a run mean nothing; what it
        # exercises is the launch, the sharding, the segmented reducer with a real second rank, the gathers and the line's schema.
        rehearsal = bool(os.environ.get("CHORE_BENCH_REHEARSAL"))
        if rehearsal:
            self.local, backend = 0, "gloo"
            import faulthandler
            faulthandler.dump_traceback_later(int(os.environ.get("CHORE_BENCH_REHEARSAL_DUMP_S", "600")), repeat=True)     # where a hung rank is
        if self.world != gpus:
            raise SystemExit(f"--gpus {gpus} but WORLD_SIZE={self.world}")
        self.cuda = use_gpu and torch.cuda.is_available()
        self.dist = None
        if self.cuda:
            torch.cuda.set_device(self.local)
            self.dev = torch.device("cuda", self.local)
        else:
            self.dev = torch.device("cpu")
        if self.world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")      # one node: gloo must not try to resolve the container's hostname
            if self.cuda:
                # RCCL for device tensors (the gradient all-reduce, the fitted-parameter gather), gloo for the timing's barrier and
                # MAX on host scalars -- and NO device_id: the RCCL communicator is then created by the first device collective,
                # i.e. by the training record.  A live communicator costs the query record most of what two batches in flight buy
                # (4.74 -> 5.09 ms per step with a communicator merely initialised: scripts/inflight_rccl_probe.py).
                dist.init_process_group(backend=backend or "cpu:gloo,cuda:nccl", init_method="env://")
            else:
                dist.init_process_group(backend=backend or "gloo", init_method="env://")
            self.dist = dist
        # N = 1: a one-rank RCCL process group, so that the training record runs the reference's DDP wrap (train_launch.py:30)
        # with its bucketed all-reduce on RCCL's stream on ONE GPU too (the collective executes; no xGMI traffic with one rank).
        # The timing helpers above keep `self.dist = None`: no barrier / MAX collective inside the N = 1 timed regions.
        self.group1, self.group1_error = None, None
        if self.world == 1 and one_rank_group and self.cuda:
            import torch.distributed as dist
            try:
                if not dist.is_initialized():
                    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
                    if "MASTER_PORT" not in os.environ:
                        s = socket.socket()
                        s.bind(("127.0.0.1", 0))
                        os.environ["MASTER_PORT"] = str(s.getsockname()[1])
                        s.close()
                    dist.init_process_group(backend=backend or "cpu:gloo,cuda:nccl", init_method="env://", rank=0, world_size=1)   # lazy, see above
                self.group1 = dist
            except Exception as e:      # the record then says so ("grad_allreduce": "none ..."); the bench line itself must not die here
                self.group1_error = repr(e)

    def barrier(self):
        if self.dist is not None:
            if self.cuda:       # on a host tensor: gloo (a device barrier would instantiate the RCCL communicator)
                self.dist.all_reduce(torch.zeros(1))
            else:
                self.dist.barrier()

    def sync(self):
        if self.cuda:
            torch.cuda.synchronize()

    def max_over_ranks(self, seconds):
        if self.dist is None:
            return seconds
        t = torch.tensor([seconds], dtype=torch.float64)          # host tensor: gloo
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def timed(self, step, steps, warmup):
        """the contract's timing: W untimed steps, then exactly K between barrier + synchronize, MAX over ranks"""
        for _ in range(warmup):
            step()
        self.barrier()
        self.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        self.sync()
        self.barrier()
        return self.max_over_ranks(time.perf_counter() - t0)

    def close(self):
        if self.dist is not None:
            self.dist.destroy_process_group()
        elif self.group1 is not None:
            self.group1.destroy_process_group()


def base_line(args, ctx, metric, value, unit, elapsed, higher, dtype, config):
    return {"metric": metric, "value": value, "unit": unit, "n_gpus": ctx.world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": higher, "scaling": "weak", "vs_baseline": None,
            "dtype": dtype, "data": "synthetic", "config": config}


# ---- the stdout line ---------------------------------------------------------------------------------------------------
# The driver parses ONE JSON line from a bounded capture of stdout (round 5's 25 KB line left BENCH_r05.parsed null).  The
# stdout line is therefore the contract's keys only, hard-capped; every other measurement of the run goes to
# bench_detail.json (next to bench.py, and under gpurun_out/ so that it travels back from a GPU box) and to stderr.
LINE_LIMIT = 6000
_TOP_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
             "dtype", "data")
_ROOF_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms")
_CPU_KEYS = ("value", "unit", "cores", "kind", "sample")
_CFG_KEYS = ("workload", "images_per_gpu", "points_per_image", "batches_in_flight", "frames_per_gpu", "frames",
             "adam_iterations_per_step", "global_batch", "parallelism", "reducer")


def _clip(v, n):
    if isinstance(v, str) and len(v) > n:
        return v[:n - 1] + "~"
    if isinstance(v, float):
        return float("%.6g" % v)
    return v


def _pick(d, keys, n):
    return {k: _clip(d[k], n) for k in keys if isinstance(d, dict) and k in d}


def slim_line(out, text=160):
    """the driver-facing line: the contract's keys of the headline, and of each record {value, unit, ms_per_step, dtype,
    config.workload, roofline.frac, cpu_baseline.value}; `text` bounds every string"""
    line = _pick(out, _TOP_KEYS, text)
    line["config"] = _pick(out.get("config", {}), _CFG_KEYS, text)
    if "roofline" in out:
        line["roofline"] = _pick(out["roofline"], _ROOF_KEYS, text)
    if "cpu_baseline" in out:
        line["cpu_baseline"] = _pick(out["cpu_baseline"], _CPU_KEYS, text)
    for k in ("single_in_flight_ms_per_step", "query_ms", "encode_ms", "query_fwd_bwd_points_per_s", "query_only_points_per_s",
              "surface_step_points_per_s"):
        if k in out:
            line[k] = _clip(out[k], text)
    for name in ("train", "fit", "fit_fp16_fields"):
        rec = out.get(name)
        if not isinstance(rec, dict):
            continue
        if "error" in rec:
            line[name] = {"error": _clip(rec["error"], text)}
            continue
        sub = _pick(rec, ("metric", "value", "unit", "ms_per_step", "dtype", "higher_is_better", "steps", "warmup"), text)
        sub["config"] = _pick(rec.get("config", {}), ("workload",), text)
        if isinstance(rec.get("roofline"), dict):
            sub["roofline"] = _pick(rec["roofline"], ("bound", "achieved", "peak", "unit", "frac", "traffic"), text)
        if isinstance(rec.get("cpu_baseline"), dict):
            sub["cpu_baseline"] = _pick(rec["cpu_baseline"], _CPU_KEYS, text)
        if isinstance(rec.get("allreduce"), dict):
            sub["allreduce"] = _pick(rec["allreduce"], ("ms_per_step_synced", "ms_per_step_no_sync", "share_of_step"), text)
        line[name] = sub
    if "records_aborted" in out:
        line["records_aborted"] = _pick(out["records_aborted"], ("stage", "after_s"), text)
    line["detail"] = "bench_detail.json"
    return line


def emit_line(out, stream):
    """write the full record to bench_detail.json (+ stderr) and ONE bounded JSON line to `stream`"""
    full = json.dumps(out)
    here = os.path.dirname(os.path.abspath(__file__))
    for d in (here, os.path.join(here, "gpurun_out")):
        try:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "bench_detail.json"), "w") as f:
                f.write(full + "\n")
        except OSError as e:
            print("[bench] could not write bench_detail.json in %s: %r" % (d, e), file=sys.stderr, flush=True)
    print("[bench detail] " + full, file=sys.stderr, flush=True)
    text = 160
    line = slim_line(out, text)
    while len(json.dumps(line)) > LINE_LIMIT and text > 20:
        text //= 2
        line = slim_line(out, text)
    s = json.dumps(line)
    assert len(s) <= LINE_LIMIT, "bench line of %d bytes" % len(s)
    print(s, file=stream, flush=True)


DUMP_LIMIT_BYTES = 64 * 10 ** 6


def dump_outputs(d, named):
    """--dump-outputs: each tensor of `named` as d/<name>.npy in float32.  Over DUMP_LIMIT_BYTES in all, the same seeded
    sample of the last axis (the points) is written for every tensor -- the same arguments give the same sample."""
    os.makedirs(d, exist_ok=True)
    arrays = {k: t.detach().float().cpu().numpy() for k, t in named.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        n = min(a.shape[-1] for a in arrays.values())
        keep = np.sort(np.random.RandomState(0).choice(n, n * DUMP_LIMIT_BYTES // total, replace=False))
        arrays = {k: np.ascontiguousarray(a[..., keep]) for k, a in arrays.items()}
    for k, a in arrays.items():
        np.save(os.path.join(d, k + ".npy"), a)


# ---- mode: query ------------------------------------------------------------------------------------------------------
def mode_query(args, ctx):
    from chore_amd import _lib
    from chore_amd.model import CHORE
    from chore_amd.utils import synth
    from chore_amd.utils.field_check import field_errors
    dev, rank, local = ctx.dev, ctx.rank, ctx.local
    B, N = args.batch, args.points

    def make(dtype, seed_rank):
        opt = chore_opt(dtype)
        opt.gpu_id = local
        net = CHORE(opt).to(dev).eval()
        synth.load_synth_weights(net, seed=0)
        for p in net.parameters():
            p.requires_grad_(False)
        images = torch.from_numpy(synth.synth_images(B, 512, 512, seed=seed_rank)).to(dev)
        points = torch.from_numpy(synth.synth_points(B, N, seed=1 + seed_rank)).to(dev)
        cc = torch.tensor([synth.CROP_CENTER] * B, dtype=torch.float32, device=dev)

        def step():
            net.filter(images)
            net.query(points, crop_center=cc)
        return net, images, points, cc, step

    def headline(elapsed, issue, in_flight, **config):
        return base_line(args, ctx, "query-points/sec (HGFilters encode + 20k-pt MLP field query per 512x512 image)",
                         ctx.world * B * N * args.steps / elapsed, "points/s", elapsed, True, args.dtype,
                         dict({"workload": "BASELINE configs[1]: encode %dx(5,512,512) + query %dx%d points per GPU per step"
                                           % (B, B, N),
                               "precision": {"fp16x3": "fp32 tensors; the encoder's convolutions as three fp16 MFMAs per product on hi/lo "
                                                       "split operands, fp32 accumulation (fp32-grade: meets the 1e-4 field tolerance); "
                                                       "BASELINE names bf16 for this config -- that mode is in other_modes with its error",
                                             "bf16": "bf16 feature maps and MFMA operands in the encoder, fp32 accumulation (a 1e-2 mode); heads fp32-grade",
                                             "fp16": "IEEE half feature maps (BASELINE configs[4]'s 'fp16 fields'); convolutions as two fp16 MFMAs per "
                                                     "product (activation x weight hi, lo), fp32 accumulation (a 1e-3 mode); heads fp32-grade",
                                             "fp32": "fp32 tensors, native fp32 MFMA"}[args.dtype],
                               "images_per_gpu": B, "points_per_image": N, "image": "512x512x5", "step_issue": issue,
                               "batches_in_flight": in_flight,
                               "heads_dtype": "fp32 results on the fp16 matrix cores, hi/lo split operands" if args.dtype != "fp32"
                                              else "fp32 (native fp32 MFMA)", "sharding": "images across ranks, no collective"},
                              **config))

    net, images, points, cc, step = make(args.dtype, rank)
    with torch.no_grad():
        # The timed step is ONE hipGraph replay of filter + query (captured once after a warm-up on the capture stream; images and
        # points live in static device buffers, which is what a serving loop copies its next batch into): the same ~170 launches
        # without the host in the loop.  --eager-step issues them from Python instead (eager_ms_per_step reports that either way).
        # --in-flight K (default 2): K recordings of the step, each with its own activation workspace and outputs, replayed round
        # robin on K streams -- batch i+1's encode starts while batch i is still running, which is how a fitting / serving loop
        # with double-buffered batches drives the device.  One step alone leaves the chip partly idle (dependent launches, tails of
        # ~256-workgroup kernels): 5.27 -> 4.78 ms per step with two in flight, same outputs bit for bit
        # (`pipelined_outputs_equal_eager`).  `single_in_flight_ms_per_step` is the one-recording number.
        run, issue = step, "eager launches from Python"
        single_elapsed, pipe_ok, graphs = None, None, []
        if not args.eager_step:
            try:
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(2):
                        step()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize()
                _drain()
                for k in range(max(1, args.in_flight)):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):     # own capture stream = own encoder workspace
                        step()
                    graphs.append((g, torch.cuda.current_stream(dev) if k == 0 else torch.cuda.Stream(dev), net.get_preds()))
                step_graph = graphs[0][0]
                counter = [0]

                def run_pipelined():
                    g, s, _ = graphs[counter[0] % len(graphs)]
                    counter[0] += 1
                    with torch.cuda.stream(s):
                        g.replay()
                if len(graphs) > 1:
                    # Which stream the second recording is replayed on matters: streams share a handful of hardware queues, and on
                    # a queue shared with the first recording's work the two steps run one after the other (5.1 - 5.6 ms per step
                    # over ten candidate streams in one process, scripts/half_batch_probe.py).  Warm-up calibration: a few pairs
                    # per candidate stream, the fastest one is kept.
                    def round_ms(k, sk, n=4):          # recordings 0 .. k round robin, recording k on candidate stream sk
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(n):
                            for j in range(k + 1):
                                with torch.cuda.stream(sk if j == k else graphs[j][1]):
                                    graphs[j][0].replay()
                        torch.cuda.synchronize()
                        return (time.perf_counter() - t0) / ((k + 1) * n)
                    for k in range(1, len(graphs)):
                        # Round 5: NO calibration by default -- over 5 process starts the two-in-flight step read 4.518 .. 4.543 ms with the
                        # calibration and 4.523 .. 4.528 ms without (profiles/r05_headline_variance.txt): the unlucky stream pairs of
                        # round 4 did not occur on this runtime.  CHORE_BENCH_CALIBRATE=1 brings the eight-candidate search back.
                        cands = [graphs[k][1]] + [torch.cuda.Stream(dev) for _ in range(7 if os.environ.get("CHORE_BENCH_CALIBRATE") else 0)]
                        for c in cands:
                            round_ms(k, c, 1)
                        best = min(cands, key=lambda c: round_ms(k, c))
                        graphs[k] = (graphs[k][0], best, graphs[k][2])
                    run = run_pipelined
                    issue = ("%d recordings of the step (filter + query, own workspace and outputs each) replayed round robin on %d streams: "
                             "%d batches in flight; static input buffers" % (len(graphs), len(graphs), len(graphs)))
                else:
                    run, issue = step_graph.replay, "one hipGraph replay per step (filter + query captured once; static input buffers)"
            except Exception as e:
                torch.cuda.synchronize()
                graphs = []
                issue = "eager launches from Python (graph capture failed: %s)" % repr(e)[:120]
        elapsed = ctx.timed(run, args.steps, args.warmup)
        if args.dump_outputs and rank == 0:
            # the outputs of the last timed step: the recording the round robin replayed last, the one recording, or the eager step's
            if len(graphs) > 1:
                preds = graphs[(counter[0] - 1) % len(graphs)][2]
            else:
                preds = graphs[0][2] if graphs else net.get_preds()
            dump_outputs(args.dump_outputs, dict(zip(("df", "pca", "parts", "centers"), preds)))
        if not args.full:
            return headline(elapsed, issue, max(1, len(graphs))) if rank == 0 else None
        if len(graphs) > 1:
            single_elapsed = ctx.timed(graphs[0][0].replay, args.steps, 2)
            # every recording's outputs against an eager step's, after one more pipelined round
            step()
            torch.cuda.synchronize()
            want = [t.clone() for t in net.get_preds()]
            for _, _, preds in graphs:
                for t in preds:
                    t.zero_()
            for _ in graphs:
                run()
            torch.cuda.synchronize()
            pipe_ok = all(torch.equal(a, b) for _, _, preds in graphs for a, b in zip(preds, want))
        eager_elapsed = ctx.timed(step, args.steps, 2)

        # the same two timings once more at the END of the run (mode_all calls it after the training record, i.e. with an RCCL
        # communicator alive in the process): what a DDP / serving process that holds a communicator sees
        def retime(_keep=(net, images, points, cc, step)):     # (a recorded graph holds ADDRESSES, not references: keep what it reads alive)
            with torch.no_grad():
                r = {"ms_per_step": ctx.timed(run, args.steps, 3) / args.steps * 1e3}
                if len(graphs) > 1:
                    r["single_in_flight_ms_per_step"] = ctx.timed(graphs[0][0].replay, args.steps, 2) / args.steps * 1e3
            return r
        if not os.environ.get("CHORE_BENCH_NO_REQUERY"):
            ctx.requery = retime

        # ---- component timings + live roofline measurement (outside the timed region) ----
        def timed(fn, n):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n

        enc_ms = timed(lambda: net.filter(images), 5)
        qry_ms = timed(lambda: net.query(points, crop_center=cc), 20)
        _lib.profile_enable(local, True)
        for _ in range(3):
            net.filter(images)
        prof = _lib.profile_read(local)
        _lib.profile_enable(local, False)
        # ---- field values against the reference's (rank 0 inputs are the golden's) ----
        field_err, other_modes = None, {}
        if rank == 0 and B == 4 and N == 20000:
            step()
            field_err = field_errors(net.get_preds())
            try:      # all 80 000 points, through the reference's sums over blocks of 32 points (tests/golden/config2_blocksums.npz)
                from chore_amd.utils.field_check import block_errors
                field_err["all_points_block_means"] = block_errors(net.get_preds())
            except Exception as e:
                field_err["all_points_block_means"] = {"error": repr(e)[:120]}
            for mode in ("fp16", "bf16", "fp16x3", "fp32"):
                if mode == args.dtype:
                    continue
                net2, _, _, _, step2 = make(mode, 0)
                for _ in range(2):
                    step2()
                t2 = timed(step2, 5)
                other_modes[mode] = {"ms_per_step": t2, "value": B * N / t2 * 1e3, "unit": "points/s",
                                     "step_issue": "eager launches from Python, one step at a time",
                                     "field_err": field_errors(net2.get_preds())["all"]}
                try:        # the same step as ONE hipGraph replay (what `single_in_flight_ms_per_step` is for the headline mode)
                    torch.cuda.synchronize()
                    _drain()
                    g2 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g2):
                        step2()
                    for _ in range(3):
                        g2.replay()
                    t3 = timed(g2.replay, 20)
                    other_modes[mode].update(replayed_ms_per_step=t3, replayed_points_per_s=B * N / t3 * 1e3)
                    del g2
                except Exception as e:
                    torch.cuda.synchronize()
                    other_modes[mode]["replayed_error"] = repr(e)[:120]
                del net2
    # metric 1(ii): forward + backward to the points (the generator's projection step, recon/generator.py:50-79)
    pg = points.clone().requires_grad_(True)

    def fwd_bwd():
        pg.grad = None
        net.query(pg, crop_center=cc)
        torch.clamp(net.get_preds()[0][:, 0], max=2.0).sum().backward()
    for _ in range(3):
        fwd_bwd()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fwd_bwd()
    e1.record()
    torch.cuda.synchronize()
    fb_ms = e0.elapsed_time(e1) / 10
    # the same step as the generator issues it (Generator.approx_surface: CHORE.surface_step = chore_gen_surface_step_fused -- the
    # distance head's forward, its clamp mask, the backward to the points and the projection in ONE launch; None in the fp32-MFMA mode)
    surf_ms = None
    with torch.no_grad():
        if net.surface_step(points, cc, 0, 2.0) is not None:
            torch.cuda.synchronize()
            e0.record()
            for _ in range(10):
                net.surface_step(points, cc, 0, 2.0)
            e1.record()
            torch.cuda.synchronize()
            surf_ms = e0.elapsed_time(e1) / 10

    # SURVEY 8(d) metric 1: points/s = B * N / MEDIAN latency over >= 100 hipGraph replays, (i) query forward, (ii) forward +
    # backward to the points (the generator's step), (iii) the encoder; the whole step as one graph beside them
    def graph_median(fn, replays=100):
        try:
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            _drain()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            for _ in range(5):
                g.replay()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(replays)]
            for a, b in evs:
                a.record()
                g.replay()
                b.record()
            torch.cuda.synchronize()
            ts = sorted(a.elapsed_time(b) for a, b in evs)
            return {"median_ms": ts[len(ts) // 2], "p10_ms": ts[len(ts) // 10], "p90_ms": ts[(9 * len(ts)) // 10], "replays": replays}
        except Exception as e:          # a capture that fails must not take the bench line with it
            torch.cuda.synchronize()
            return {"error": repr(e)[:200]}

    with torch.no_grad():
        g_query = graph_median(lambda: net.query(points, crop_center=cc))
        g_encode = graph_median(lambda: net.filter(images))
        g_step = graph_median(step)
    g_fwd_bwd = graph_median(fwd_bwd)
    graph_replay = {"query_fwd": g_query, "query_fwd_bwd_points": g_fwd_bwd, "encode": g_encode, "encode_plus_query": g_step,
                    "note": "SURVEY 8(d) metric 1: each workload captured once in a hipGraph, 100 replays, one event pair per replay"}
    for k, pts in (("query_fwd", B * N), ("query_fwd_bwd_points", B * N), ("encode_plus_query", B * N)):
        if "median_ms" in graph_replay[k]:
            graph_replay[k]["points_per_s"] = pts / graph_replay[k]["median_ms"] * 1e3
    if "median_ms" in g_encode:
        g_encode["images_per_s"] = B / g_encode["median_ms"] * 1e3
    out = None
    if rank == 0:
        kernels = {}
        for k, v in prof.items():
            if v["launches"]:
                kernels[k] = {"ms_per_step": v["ms"] / 3, "launches_per_step": v["launches"] // 3,
                              "tflops": v["flops"] / v["ms"] / 1e9 if v["flops"] else None,
                              "gbps": v["bytes"] / v["ms"] / 1e6}
        tname = TNAME[args.dtype]
        kernels = {k.replace("<T,", "<%s, " % tname).replace(",", ", ").replace(",  ", ", "): v for k, v in kernels.items()}
        # HBM-side bytes per launch of each kernel from the committed rocprofv3 counter passes (FETCH_SIZE x2 +
        # WRITE_SIZE, scripts/pmc_traffic.py) -- counters cannot be read live, so this is the last profiled build
        traffic = {}
        tpath = os.path.join(REPO, "profiles", "pmc_traffic_%s.json" % args.dtype)
        if os.path.exists(tpath):
            traffic = {k: v["bytes_per_launch"] for k, v in json.load(open(tpath)).items()}
            # (rocprofv3 prints conv_pc_kernel's last template argument -- SC, the scaled-operand instantiation of the training
            # data gradients; the library's own profile classes, which name `dom` below, do not carry it)
            traffic.update({k[:-len(", false>")] + ">": v for k, v in traffic.items() if k.startswith("conv_pc_kernel<") and k.endswith(", false>")})
            # (conv_mw_kernel's last two template arguments: GN = true, SC = false in the inference step)
            traffic.update({k[:-len(", true, false>")] + ">": v for k, v in traffic.items() if k.startswith("conv_mw_kernel<") and k.endswith(", true, false>")})
        # rocprofv3 name of the forward query kernel this size runs (csrc/query_fwd.hip: eight-wave variant for large queries,
        # 32-point tiles when 64-point tiles would not fill the CUs)
        x3 = args.dtype in ("fp16x3", "bf16", "fp16")        # heads on the fp16 matrix cores with split operands (fp32 mode: native fp32 MFMA)
        qt = "float" if args.dtype == "fp16x3" else ("qh16_t" if args.dtype == "fp16" else tname)
        small = B * ((N + 63) // 64) <= 256
        if x3 and not os.environ.get("CHORE_QUERY_X3_NOSPLIT"):     # fp16 x 3 heads: two waves per head (csrc/query_fwd.hip)
            qname = "query_fwd_x3_split_kernel<%s, %d>" % (qt, 1 if small else 2)
        elif small:
            qname = "query_fwd_f32_kernel<%s, 1, false, %s>" % (qt, "true" if x3 else "false")
        elif x3:        # four waves, two column blocks each (the eight-wave kernel is bound by the L1 there)
            qname = "query_fwd_f32_kernel<%s, 2, false, true>" % qt
        else:
            qname = "query_fwd_f32_w8_kernel<%s, false, false>" % qt
        kernels[qname] = {"ms_per_step": qry_ms, "launches_per_step": 1,
                          "tflops": HEADS_FLOP_PER_POINT * B * N / qry_ms / 1e9, "gbps": None}
        dom = max((k for k in kernels if kernels[k]["tflops"]), key=lambda k: kernels[k]["ms_per_step"])
        dv = kernels[dom]
        dom_dtype = ("fp16x3" if x3 else "fp32") if dom == qname else args.dtype     # the heads: fp16 x 3, or the fp32 MFMA in fp32 mode
        roof = {"kernel": dom, "bound": "mfma", "achieved": dv["tflops"], "peak": PEAK_TFLOPS[dom_dtype],
                "unit": "TFLOP/s", "frac": dv["tflops"] / PEAK_TFLOPS[dom_dtype], "traffic": traffic.get(dom),
                "traffic_source": "profiles/pmc_traffic_%s.json (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, bytes/launch)"
                                  % args.dtype if dom in traffic else None,
                "avg_launch_ms": dv["ms_per_step"] / dv["launches_per_step"],
                "flops_per_launch": dv["tflops"] * 1e9 * dv["ms_per_step"] / dv["launches_per_step"]}
        if dom_dtype == "fp16x3":     # every algorithmic product is three fp16 MFMAs: the share of the matrix cores' issue rate
            roof["mfma_issue_frac"] = 3.0 * roof["frac"]
        out = headline(elapsed, issue, max(1, len(graphs)), field_err=field_err,
                       field_err_note="max / mean absolute and relative-L2 difference to the values THE REFERENCE "
                                      "produced for the same images and points (tests/golden/config2_fields.npz): 768 "
                                      "of the 20 000 points of each of the 4 images are reference-checked value by value; "
                                      "field_err.all_points_block_means covers ALL 80 000 points through the reference's sums "
                                      "over blocks of 32 consecutive points (tests/golden/config2_blocksums.npz): the largest "
                                      "deviation of a block's mean; stated tolerances: chore_amd/utils/field_check.py")
        single_ms = None if single_elapsed is None else single_elapsed / args.steps * 1e3
        out.update({"roofline": roof, "other_modes": other_modes, "encode_ms": enc_ms, "query_ms": qry_ms,
                    "eager_ms_per_step": eager_elapsed / args.steps * 1e3,
                    "single_in_flight_ms_per_step": single_ms,
                    "single_in_flight_points_per_s": None if single_ms is None else B * N / single_ms * 1e3,
                    "headline_is": ("`value` = throughput with %d batches in flight (two recordings of the SAME full step on two streams, "
                                    "outputs bit-equal to eager); one step at a time is single_in_flight_*; both measured without an RCCL "
                                    "communicator in the process (rccl_communicator_alive: false) -- `with_rccl_communicator` repeats both "
                                    "after the training record has created one" % max(1, len(graphs))),
                    "rccl_communicator_alive": False,
                    "pipelined_outputs_equal_eager": pipe_ok,
                    "query_only_points_per_s": B * N / qry_ms * 1e3,
                    "query_fwd_bwd_points_per_s": B * N / fb_ms * 1e3, "query_fwd_bwd_ms": fb_ms,
                    "surface_step_ms": surf_ms, "surface_step_points_per_s": (B * N / surf_ms * 1e3) if surf_ms else None,
                    "encode_tflops": B * ENCODER_FLOP_PER_IMAGE_EVAL / enc_ms / 1e9,
                    "encode_flop_per_image": ENCODER_FLOP_PER_IMAGE_EVAL, "graph_replay": graph_replay, "kernels": kernels})
        if ctx.world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_query()
            out["cpu_baseline_torch"] = cpu_baseline_query_torch()
    return out


# ---- mode: fit --------------------------------------------------------------------------------------------------------
def fit_batch_inputs(B, seed, dev):
    """one loader batch of the data/test_data.py contract: 512x512 RGB + a person and an object mask, crop metadata"""
    from chore_amd.utils import synth
    img = synth.synth_images(B, 512, 512, seed=seed)
    img[:, 3:] = 0
    img[:, 3, 120:420, 180:300] = 1          # person mask
    img[:, 4, 250:380, 280:420] = 1          # object mask
    img[:, :3] *= np.maximum(img[:, 3:4], img[:, 4:5])      # background zeroed like data/base_data.py:179-192
    cc = torch.tensor([synth.CROP_CENTER] * B, dtype=torch.float32)
    return dict(images=torch.from_numpy(img).to(dev), path=[f"/synthetic/seq{seed}/t{i:04d}.000/k1.color.jpg" for i in range(B)],
                crop_center=cc.to(dev), old_crop_center=cc.clone(), resize_scale=torch.ones(B), crop_scale=torch.ones(B))


SMPL_ITERS = dict(iter_for_betas=1, iter_for_pose=1, iter_for_kpts=1, steps_per_iter=10, max_iter=7)      # 10 x 10 = 100
OBJECT_ITERS = dict(obj_iter=5, sil_iter=5, joint_iter=5, max_iter=5, steps_per_iter=10)                    # 20 x 10 = 200


def mode_fit(args, ctx):
    from chore_amd.model import CHORE
    from chore_amd.parallel.frame_shard import gather_fitted
    from chore_amd.recon.assets import SyntheticAssets
    from chore_amd.recon.generator import Generator
    from chore_amd.recon.recon_fit_behave import ReconFitterBehave
    from chore_amd.utils import synth
    dev, rank = ctx.dev, ctx.rank
    B = args.frames_per_gpu or (1 if ctx.world == 1 else 8)     # configs[2]: one frame; configs[4]: 64 frames on 8 GPUs
    opt = chore_opt(args.dtype)
    opt.gpu_id = ctx.local
    net = CHORE(opt).to(dev).eval()
    synth.load_synth_weights(net, seed=0)
    fitter = ReconFitterBehave(None, device=dev, obj_name="synthetic", outpath=None, args=opt, assets=SyntheticAssets(0))
    fitter.use_graphs = not args.eager
    fitter.reuse_graphs = not args.eager and not os.environ.get("CHORE_FIT_NO_REUSE")    # recorded steps kept across chains (same shapes)
    net.image_filter.static_outputs = fitter.reuse_graphs
    fitter.early_stop = False      # time exactly 300 iterations (with random weights the rule fires at once)
    fitter.timer = []
    # random weights have no thin zero level set: a loose filter collects the 5 000 points in the first rounds
    gen = Generator(net, None, threshold=2.0, sparse_thres=0.03, filter_val=1.0, device=dev)
    data = fit_batch_inputs(B, rank, dev)
    stages = {}
    chains = []          # per timed chain: {stage: wall ms}

    def clock(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        stages[name] = stages.get(name, 0.0) + ms
        if chains:
            chains[-1][name] = chains[-1].get(name, 0.0) + ms
        return out

    result = {}

    def step():
        chains.append({})
        pc = clock("generate_pclouds", lambda: gen.generate_pclouds_batch(data, num_points=5000, num_steps=10, mute=True))
        (betas_dict, body_kpts, human_parts, human_points, human_t, obj_points, part_colors, part_labels, query_dict,
         smpl) = clock("prep_smplfit", lambda: fitter.prep_smplfit(data, gen, pc))
        smpl, scale = clock("optimize_smpl", lambda: fitter.optimize_smpl(smpl, betas_dict, **SMPL_ITERS))
        obj_R, obj_s, obj_t, object_init = clock("init_obj_fit_data", lambda: fitter.init_obj_fit_data(B, human_t, pc, scale))
        dd = {"obj_R": obj_R, "obj_t": obj_t, "obj_s": obj_s, "objects": object_init, "smpl": smpl, "images": data["images"],
              "body_kpts": body_kpts, "query_dict": query_dict, "part_labels": part_labels}
        clock("optimize_smpl_object", lambda: fitter.optimize_smpl_object(net, dd, **OBJECT_ITERS))
        result.update(trans=smpl.trans.detach(), obj_t=obj_t.detach(), obj_s=obj_s.detach())

    for _ in range(args.warmup):
        step()
    stages.clear()
    chains.clear()
    fitter.timer.clear()
    elapsed = ctx.timed(step, args.steps, 0)
    iters = sum(t[2] for t in fitter.timer)
    iter_ms = sum(t[0].elapsed_time(t[1]) for t in fitter.timer) / iters
    iter_ms = ctx.max_over_ranks(iter_ms)
    # SURVEY 8(d) metric 2: MEDIAN ms per step per phase.  One sample = one outer iteration (steps_per_iter inner steps between
    # two events) of one chain; `chains` timed chains x (10 outer iterations of optimize_smpl, 5 + 5 + 10 of optimize_smpl_object)
    by_phase = {}
    for e0, e1, n, ph in fitter.timer:
        by_phase.setdefault(ph or "?", []).append(e0.elapsed_time(e1) / n)
    per_phase = {ph: {"median_ms_per_iter": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                      "samples": len(v), "iterations": len(v) * SMPL_ITERS["steps_per_iter"]} for ph, v in by_phase.items()}
    chain_wall = [sum(c.values()) for c in chains]
    fitted = gather_fitted(result, B * ctx.world, rank, ctx.world, device=dev)
    # ---- the loop over loader batches (recon_fit_behave.py:41-76): serial, batch k+1 prepared ahead, whole chains side by side
    # (round 5).  12 consecutive batches through fit_recon, three passes each (recordings, allocator warm-up, timed) ----
    loop = {}
    if fitter.reuse_graphs and not args.eager:
        fitter.smpl_iters, fitter.object_iters, fitter.batch_seed = SMPL_ITERS, OBJECT_ITERS, 1234
        batches = [fit_batch_inputs(B, 100 + rank * 16 + k, dev) for k in range(int(os.environ.get("CHORE_BENCH_LOOP_BATCHES", "24" if B == 1 else "12")))]
        for name, pipe in (("serial", False), ("pipelined", True), ("chains", "chains")):
            marks = []

            class Loader(list):
                pass
            try:
                for rep in range(3):               # first pass: recordings; second: allocator warm-up of the concurrent pattern; third: timed
                    fitter.batch_ends = []
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    # (fit_recon shards the loader's batches rank::world under torch.distributed: every batch world times, so that
                    # each rank fits one copy of each)
                    fitter.fit_recon(opt, loader=Loader([b for b in batches for _ in range(ctx.world)]), generator=gen, save=False, pipeline=pipe)
                    torch.cuda.synchronize()
                    marks.append((time.perf_counter() - t0) * 1e3)
                ends = fitter.batch_ends
                fitter.batch_ends = None
                # Steady state = device time from the end of the first wave of batches (one per chain side by side; serial /
                # pipelined: the first batch) to the last batch's end, over the batches that ended in between.  The ends are put in
                # time order first (side by side, batches do not end in loader order), so the span is never negative; nothing is
                # derived from gaps between individual ends (interleaved chains end in bunches: round 5's medians were negative).
                wave = fitter.chains if name == "chains" else 1
                tt = sorted(ends[0].elapsed_time(e) for e in ends)
                span = (tt[-1] - tt[wave - 1]) / (len(tt) - wave) if len(tt) > wave else float("nan")
                assert not (span < 0), (name, tt)
                loop[name] = {"ms_per_batch": marks[2] / len(batches), "ms_per_frame": marks[2] / (len(batches) * B),
                              "steady_state_ms_per_batch": span, "steady_state_ms_per_frame": span / B,
                              "batches_in_span": len(tt) - wave, "first_pass_ms_per_batch": marks[0] / len(batches),
                              "batches": len(batches)}
            except Exception as e:
                loop[name] = {"error": repr(e)[:300]}
                torch.cuda.synchronize()
    out = None
    if rank == 0:
        per_step = {k: v / args.steps for k, v in stages.items()}
        # points through the heads in the 300 iterations (recon_fit_behave.py:293-337, 165-222): optimize_smpl queries the 6 890
        # vertices (forward + backward) 100 times; object-only 2 x 3 000 points (fwd + bwd) 50 times; silhouette 3 000
        # (fwd) 50 times; joint 2 x 3 000 (fwd + bwd) + 6 890 (fwd) 100 times
        fwd_pts = 100 * 6890 + 50 * 6000 + 50 * 3000 + 100 * (6000 + 6890)
        bwd_pts = 100 * 6890 + 50 * 6000 + 100 * 6000
        flops = B * (fwd_pts + bwd_pts) * HEADS_FLOP_PER_POINT / 300
        hd = "fp32" if args.dtype == "fp32" else "fp16x3"          # arithmetic of the heads (query kernels)
        out = base_line(args, ctx, "ms per fit iteration (SMPL-H LBS + field queries + loss terms + Adam; whole fit_recon chain run)",
                        iter_ms, "ms", elapsed, False, args.dtype,
                        {"workload": "%s: fit_recon chain on %d frame(s) per GPU, 300 Adam iterations = optimize_smpl "
                                     "%s + optimize_smpl_object %s" % (
                                         "BASELINE configs[2]" if (ctx.world == 1 and B == 1) else
                                         ("BASELINE configs[4] (64 frames on 8 GPUs)" if ctx.world * B == 64 else
                                          "the per-GPU share of BASELINE configs[4] (8 frames per GPU)" if B == 8 else "frame-sharded fit"),
                                         B, SMPL_ITERS, OBJECT_ITERS),
                         "frames_per_gpu": B, "frames": B * ctx.world, "adam_iterations_per_step": iters // max(args.steps, 1),
                         "inner_iteration": "eager" if args.eager else "hipGraph replay (chore_amd/recon/graph_step.py); the recorded steps "
                                            "are kept across chains of the same shapes (recon_fit_behave._FitSlot)",
                         "early_stop": "off (a fixed 300 iterations are timed)",
                         "terms": "df_h, part, pose/hand priors, smplz, pinit, j2d | object, scale, ocent | silhouette (HIP "
                                  "rasteriser), trans | contact, collision",
                         "value_is": "device time between events around the inner iterations / number of iterations; "
                                     "chain_ms_per_step holds the wall time of every stage incl. graph capture",
                         "sharding": "frames across ranks, no collective in the loop; one gather of the fitted parameters"})
        out.update({"chain_ms_per_step": per_step, "chains_timed": len(chains),
                    "chain_ms_median": float(np.median(chain_wall)), "chain_ms_all": [round(c, 2) for c in chain_wall],
                    "chain_stage_ms_median": {k: float(np.median([c.get(k, 0.0) for c in chains])) for k in per_step},
                    "per_phase": per_phase,
                    "loader_loop": dict(loop, note="fit_recon over 24 (one frame per batch) / 12 (eight) consecutive loader batches of the same shapes (recordings kept), three "
                                                   "passes (recordings; allocator warm-up; timed): ms_per_batch = wall time of the THIRD pass / batches; pipelined = batch k+1's encoder + point clouds + SMPL-H "
                                                   "initialisation on a second stream / host thread while batch k is optimised, results equal to "
                                                   "the serial loop bit for bit (tests/test_gpu_fit_chain.py); chains = the whole chains of `ReconFitterBehave.chains` (3) batches side by side, each "
                                                   "on its own stream and host thread, same results; steady_state_* = device time from the end of the first wave of batches (one "
                                                   "per chain; serial / pipelined: the first batch) to the last end / batches that ended in between"),
                    "per_phase_note": "SURVEY 8(d) metric 2: median device ms per Adam iteration per phase over all outer iterations "
                                      "of all timed chains ('global' / 'smpl all pose' / 'kpts' = optimize_smpl; 'object only' / "
                                      "'sil' / 'joint' = optimize_smpl_object, joint incl. contact + collision terms)",
                    "frame_iterations_per_s": ctx.world * B * 1e3 / iter_ms,
                    "frames_per_s_whole_chain": ctx.world * B * args.steps / elapsed,
                    "roofline": {"kernel": "whole fit iteration (field queries dominate: query_fwd_x3_split_kernel / query_bwd_f32_kernel, "
                                           "32-point tiles)", "bound": "mfma", "achieved": flops / iter_ms / 1e9,
                                 "peak": PEAK_TFLOPS[hd], "unit": "TFLOP/s", "frac": flops / iter_ms / 1e9 / PEAK_TFLOPS[hd],
                                 "frac_of_fp32_mfma_peak": flops / iter_ms / 1e9 / PEAK_TFLOPS["fp32"],
                                 "traffic": None, "flops_per_iteration": flops,
                                 "note": "algorithmic FLOPs of the heads only (600 832 per point forward, the same again backward) "
                                         "against the peak of the unit the heads run on: the fp16 matrix cores with hi/lo split "
                                         "operands (three MFMAs per product) unless the mode is fp32; a fit iteration is a chain "
                                         "of ~30-60 small dependent launches, not a matrix-core workload"},
                    "gathered": {k: list(v.shape) for k, v in fitted.items()}})
        if ctx.world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_fit()
    return out


# ---- mode: train ------------------------------------------------------------------------------------------------------
def train_grad_error(mode, dev):
    """gradient error of a training mode against THE REFERENCE's autograd on the golden batch (tests/golden/train_grads.npz: every
    trained tensor's L2 norm, and the complete gradient of every small tensor -- GroupNorm affines, biases): the deviation of the
    norms over all 475 tensors and the relative L2 error of the small tensors (what tests/test_gpu_encoder.py bounds per mode)"""
    from chore_amd.model import CHORE
    from chore_amd.utils import synth
    gdir = os.path.join(REPO, "tests", "golden")
    g, gg = np.load(os.path.join(gdir, "train_loss.npz")), np.load(os.path.join(gdir, "train_grads.npz"))
    net = CHORE(chore_opt(mode)).to(dev)
    synth.load_synth_weights(net, seed=0)
    net.train(True)
    keys = ("images", "points", "df_h", "df_o", "parts_gt", "pca_gt", "body_center", "obj_center", "crop_center")
    error, _ = net(**{k: torch.from_numpy(g[k]).to(dev) for k in keys})
    error.backward()
    params = dict(net.named_parameters())
    norm_dev, rel = [], []
    for name in [str(n) for n in gg["names"]]:
        ref = gg["s_" + name]
        if np.isnan(ref).any() or params[name].grad is None:
            continue
        a = params[name].grad.detach().float().cpu().numpy().astype(np.float64)
        norm_dev.append(abs(np.sqrt((a ** 2).sum()) - ref[2]) / ref[2])
        if "g_" + name in gg.files:
            rel.append(np.sqrt(((a - gg["g_" + name]) ** 2).sum()) / ref[2])
    return {"loss_rel_err": abs(float(error.detach()) - float(gg["error"])) / float(gg["error"]), "tensors": len(norm_dev),
            "l2_norm_rel_dev_max": float(np.max(norm_dev)), "l2_norm_rel_dev_median": float(np.median(norm_dev)),
            "small_tensor_rel_l2_median": float(np.median(rel)), "small_tensor_rel_l2_max": float(np.max(rel)),
            "against": "the reference's CPU autograd gradients of the same batch (tests/golden/train_grads.npz)"}


def _drain():
    """before a recording: no collective left in the process group's watchdog list (chore_amd.parallel.drain_collectives)"""
    from chore_amd.parallel import drain_collectives
    drain_collectives()


def _stage(ctx, what):
    """progress marks of every rank on stderr (rehearsals of the N > 1 path only)"""
    if os.environ.get("CHORE_BENCH_REHEARSAL") or os.environ.get("CHORE_BENCH_STAGES"):
        mem = torch.cuda.memory_allocated() / 2 ** 30 if ctx.cuda else 0.0
        print("[rank %d] %s (%.1f GiB allocated)" % (ctx.rank, what, mem), file=sys.stderr, flush=True)


def mode_train(args, ctx):
    from chore_amd.model import CHORE
    from chore_amd.utils import synth
    dev, rank, local = ctx.dev, ctx.rank, ctx.local
    opt = chore_opt(args.dtype)
    opt.gpu_id = local
    net = CHORE(opt).to(dev)
    synth.load_synth_weights(net, seed=0)
    net.train(True)
    net.losses_on_host = False     # the six separate losses stay on the device: no host synchronisation inside the step
    # Gradient reduction.  Default: chore_amd.parallel.FlatGradReducer -- one flat fp32 gradient arena, all-reduced
    # over RCCL in a few large chunks after the backward, mean over the ranks (the arithmetic of the reference's DDP wrap).  The
    # stock wrap (train_launch.py:30: DistributedDataParallel(find_unused_parameters=True)) is timed beside it: its per-parameter
    # hooks and bucket copies sit inside the launch-bound backward chain (profiles/r04_ddp_overhead.txt).  --reducer ddp makes it
    # the primary number.  With one GPU both run on a ONE-rank RCCL group: the collectives execute, nothing crosses xGMI.
    from chore_amd.parallel import FlatGradReducer, chore_segments
    have_group = ctx.world > 1 or ctx.group1 is not None
    reducer_kind = args.reducer if have_group else "none"
    # capturable: the step counter lives on the device, so optimizer.step() can be recorded into the step's hipGraph
    optim = torch.optim.Adam(net.parameters(), lr=1e-4, **({} if os.environ.get("CHORE_ADAM_DEFAULT") else {"fused": True, "capturable": True}))
    B, N = args.batch, args.points
    rs = np.random.RandomState(50 + rank)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    batch = dict(images=t(synth.synth_images(B, 512, 512, seed=rank)), points=t(synth.synth_points(B, N, seed=1 + rank)),
                 df_h=t(rs.uniform(0, 0.3, (B, N)).astype(np.float32)), df_o=t(rs.uniform(0, 0.3, (B, N)).astype(np.float32)),
                 parts_gt=t(rs.randint(0, 14, (B, N))), pca_gt=t(rs.standard_normal((B, 3, 3, N)).astype(np.float32)),
                 body_center=t((rs.standard_normal((B, 3)) * 0.3).astype(np.float32)),
                 obj_center=t((rs.standard_normal((B, 3, N)) * 0.3).astype(np.float32)),
                 crop_center=torch.tensor([synth.CROP_CENTER] * B, dtype=torch.float32, device=dev))
    last = {}

    def make_step(model, reducer):
        def step():
            if reducer is not None:
                reducer.zero_grad()
            else:
                optim.zero_grad(set_to_none=True)
            error, _ = model(**batch)
            error.backward()
            if reducer is not None:
                reducer.reduce()
            optim.step()
            last["err"] = error
        return step

    # round 5: the arena laid out by hourglass stack and each stack's slice all-reduced while the next stack's backward runs
    # (FlatGradReducer(segments=...) + backward_in_segments inside GraphedTrainStep); --reducer-layout flat = round 4's four
    # all-reduces after the whole backward
    # "auto": segmented when there are other ranks to exchange with; with ONE rank nothing travels, the collectives return at once and
    # the five extra graph boundaries of the segmented recording are pure cost (measured: 33.3 against 32.7 ms per step) -- the
    # N = 1 record times every layout in allreduce.variants
    layout = args.reducer_layout if args.reducer_layout != "auto" else ("segmented" if ctx.world > 1 else "flat")
    if have_group and layout == "flat":
        arena = FlatGradReducer(net)
    elif have_group:
        arena = FlatGradReducer(net, segments=chore_segments(net), collective=args.collective)
    else:
        arena = None
    step_plain = make_step(net, None)
    step_arena = make_step(net, FlatGradReducer(net) if (arena is not None and arena.segments is not None) else arena) if have_group else None
    ddp_model = None

    def step_ddp_factory():
        m = torch.nn.parallel.DistributedDataParallel(net, device_ids=[local], find_unused_parameters=True)
        return m, make_step(m, None)

    # The step is issued as hipGraph replays (chore_amd.parallel.GraphedTrainStep: forward + backward + gradient gather recorded
    # once, the RCCL all-reduce between two replays, the optimiser recorded too): ~1 600 short dependent launches per step leave
    # the device idle a quarter of the time when Python issues them.  --eager-step times the eager sequence as the primary number
    # instead; `eager_ms_per_step` reports it either way.  (Stock DDP cannot be recorded: its reducer lives in the autograd hooks.)
    from chore_amd.parallel import GraphedTrainStep
    graphed = (not args.eager_step) and reducer_kind != "ddp"

    def make_graphed(reducer):
        g = GraphedTrainStep(net, optim, reducer=reducer, warmup=2)

        def step():
            last["err"], _ = g(**batch)
        return step

    eager_primary = None
    if reducer_kind == "ddp":
        ddp_model, primary = step_ddp_factory()
    elif reducer_kind == "arena":
        primary, eager_primary = (make_graphed(arena), step_arena) if graphed else (step_arena, None)
    else:
        primary, eager_primary = (make_graphed(None), step_plain) if graphed else (step_plain, None)
    if graphed:
        args.warmup = max(args.warmup, 4)      # two eager calls, the recording, one replay: all before the timed region
    _stage(ctx, "train: primary")
    primary_fallback = None
    try:
        elapsed = ctx.timed(primary, args.steps, args.warmup)
    except Exception as e:
        # a recording that the collectives of this node's RCCL do not accept must not cost the record: the eager step with the
        # flat arena (no capture anywhere) is timed instead, and the line says so
        if not (graphed and reducer_kind == "arena"):
            raise
        import traceback
        traceback.print_exc()
        primary_fallback = repr(e)[:300]
        torch.cuda.synchronize()
        graphed, arena = False, FlatGradReducer(net)
        primary, eager_primary = make_step(net, arena), None
        elapsed = ctx.timed(primary, args.steps, 2)
    _stage(ctx, "train: eager")
    eager_elapsed = ctx.timed(eager_primary, args.steps, 2) if eager_primary is not None else None
    _stage(ctx, "train: variants")
    nosync = other = None
    variants = {}
    if have_group and reducer_kind == "arena" and graphed:
        # the same replayed step with the other reduction schemes (each its own recording, made and dropped in turn)
        for name, mk in (("flat: 4 all_reduce after the backward", lambda: FlatGradReducer(net)),
                         ("segmented all_reduce under the backward", lambda: FlatGradReducer(net, segments=chore_segments(net))),
                         ("segmented reduce_scatter + all_gather under the backward",
                          lambda: FlatGradReducer(net, segments=chore_segments(net), collective="rs_ag"))):
            try:
                _stage(ctx, "train: variant " + name)
                red = mk()
                gs = GraphedTrainStep(net, optim, reducer=red, warmup=2)
                tv = ctx.timed(lambda: gs(**batch), args.steps, 4)
                variants[name] = {"ms_per_step": tv / args.steps * 1e3}
                gs.close()
                del gs, red
            except Exception as e:
                variants[name] = {"error": repr(e)[:200]}
                _stage(ctx, "train: variant FAILED " + repr(e)[:200])
            torch.cuda.empty_cache()
    if have_group and reducer_kind == "arena":
        # the same steps without any gradient reduction, and with the reference's wrap: what the collective costs either way
        # (the DDP wrap last: its hooks stay on the parameters)
        nosync = ctx.timed(make_graphed(None) if graphed else step_plain, args.steps, 4 if graphed else 2)
        ddp_model, sd = step_ddp_factory()
        other = ("torch DistributedDataParallel(find_unused_parameters=True)", ctx.timed(sd, args.steps, 3))
    elif have_group:
        def step_nosync():
            with ddp_model.no_sync():
                primary()
        nosync = ctx.timed(step_nosync, args.steps, 2)
    out = None
    if rank == 0:
        flops = 3.0 * (B * ENCODER_FLOP_PER_IMAGE + 5 * B * N * HEADS_FLOP_PER_POINT)     # 3.82 TFLOP at B=4
        ms = elapsed / args.steps * 1e3
        out = base_line(args, ctx, "training steps/s (CHORE.forward + backward + Adam, B=4 x 512x512 images, 20k points/image per GPU)",
                        args.steps / elapsed, "steps/s", elapsed, True, args.dtype,
                        {"workload": "BASELINE configs[3]: DDP training, batch %d/GPU, %d points/image, 5 stacks" % (B, N),
                         "images_per_gpu": B, "points_per_image": N, "optimizer": "torch.optim.Adam(lr=1e-4, fused=True, capturable=True)",
                         "step_issue": ("hipGraph replays (chore_amd.parallel.GraphedTrainStep: zero_grad + forward + backward + gradient "
                                        "gather in one recording, optimizer.step() in another, the all-reduce between them)"
                                        if graphed else "eager (Python issues every launch)"),
                         "grad_allreduce": ({"arena": ("chore_amd.parallel.FlatGradReducer: flat fp32 gradient arena (%.1f MB), all-reduced "
                                                       "over RCCL (backend nccl) in %d %s, mean over ranks"
                                                       % (arena.bytes / 1e6, len(arena.chunks),
                                                          "segments (one per hourglass stack + the stem), each launched on RCCL's stream when its part "
                                                          "of the backward is done, under the rest of the backward (%s)" % args.collective
                                                          if arena.segments is not None else "chunks after the backward")) if arena is not None else "",
                                             "ddp": "torch DDP over RCCL (backend nccl), find_unused_parameters=True (the reference's wrap)"}
                                            [reducer_kind] + ("" if ctx.world > 1 else "; ONE-rank group: the collectives execute on "
                                                              "RCCL's stream, nothing crosses xGMI"))
                                           if have_group else "none (1 GPU, no process group%s)" % (
                                               ": " + ctx.group1_error if ctx.group1_error else "")})
        if primary_fallback:
            out["primary_fallback"] = {"to": "eager step, flat arena", "because": primary_fallback}
        if nosync is not None:
            out["allreduce"] = {"ms_per_step_synced": ms, "ms_per_step_no_sync": nosync / args.steps * 1e3,
                                "share_of_step": max(0.0, 1.0 - nosync / elapsed), "bytes_per_step": 4 * sum(p.numel() for p in net.parameters()),
                                "reducer": reducer_kind, "variants": variants,
                                "exposed_ms": ms - nosync / args.steps * 1e3,
                                "other_reducer": {"what": other[0], "ms_per_step": other[1] / args.steps * 1e3,
                                                  "steps_per_s": args.steps / other[1]} if other else None,
                                "world_size": ctx.world,
                                "how": "K steps without any gradient reduction against K steps with it, same model and batch"}
        if eager_elapsed is not None:
            out["eager_ms_per_step"] = eager_elapsed / args.steps * 1e3
        if other:
            # what the reference's UNCHANGED train_launch.py gets from this package: its own DistributedDataParallel wrap around the
            # eager step.  `value` needs the three-line edit of Trainer documented in INTEGRATION.md (GraphedTrainStep + FlatGradReducer).
            out["unchanged_train_launch"] = {"ms_per_step": other[1] / args.steps * 1e3, "steps_per_s": args.steps / other[1],
                                             "what": "eager step under torch DistributedDataParallel(find_unused_parameters=True), train_launch.py:30 as it is"}
        out.update({"images_per_s": ctx.world * B * args.steps / elapsed, "final_loss": float(last["err"].detach()),
                    "parameters": sum(p.numel() for p in net.parameters()),
                    "roofline": {"kernel": "whole training step (all kernels)", "bound": "mfma", "achieved": flops / ms / 1e9,
                                 "peak": PEAK_TFLOPS[args.dtype], "unit": "TFLOP/s", "frac": flops / ms / 1e9 / PEAK_TFLOPS[args.dtype],
                                 "traffic": None, "flops_per_step": flops}})
        if ctx.world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_train()
    # ---- the other precision modes of the same step (replayed, no gradient reduction), and every mode's gradient error ----
    if getattr(args, "train_other_modes", False):
        del primary, eager_primary, step_plain, step_arena, arena, ddp_model
        optim.zero_grad(set_to_none=True)
        others, errs = {}, {}
        for mode in ("fp16x3", "bf16", "fp32"):
            torch.cuda.empty_cache()
            try:
                errs[mode] = train_grad_error(mode, dev) if rank == 0 else None
            except Exception as e:
                errs[mode] = {"error": repr(e)[:200]}
            if mode == args.dtype:
                continue
            o2 = chore_opt(mode)
            o2.gpu_id = local
            net2 = CHORE(o2).to(dev)
            synth.load_synth_weights(net2, seed=0)
            net2.train(True)
            opt2 = torch.optim.Adam(net2.parameters(), lr=1e-4, fused=True, capturable=True)
            g2 = GraphedTrainStep(net2, opt2, reducer=None, warmup=2)
            n2 = 10
            t2 = ctx.timed(lambda: g2(**batch), n2, 4)
            others[mode] = {"ms_per_step": t2 / n2 * 1e3, "steps_per_s": n2 / t2, "step_issue": "hipGraph replay, no gradient reduction"}
            g2.close()
            del g2, opt2, net2
        if rank == 0:
            for mode, rec in others.items():
                rec["grad_err"] = errs.get(mode)
            out["other_modes"] = others
            out["grad_err"] = errs.get(args.dtype)
            out["precision"] = {"fp16x3": "fp32 tensors; every convolution, data gradient and weight gradient of the encoder and every GEMM of the "
                                          "heads on the fp16 matrix cores with hi / lo split operands (three MFMAs per product, fp32 accumulation): "
                                          "the reference's training precision (fp32, trainer/trainer.py:76-85) -- see grad_err",
                                "bf16": "bf16 activations and MFMA operands, fp32 accumulation, heads fp32-grade: narrower than the reference "
                                        "(grad_err: percent-level gradient error)",
                                "fp32": "fp32 tensors, native fp32 MFMA"}[args.dtype]
    return out


def mode_all(args, ctx):
    """the query line; with --full, the fit and training records inside it"""
    if not args.full:
        return mode_query(args, ctx)
    import copy
    _stage(ctx, "all: query")
    out = mode_query(args, ctx)
    _stage(ctx, "all: query done")
    subs = {}
    # training first: after the fit (a dozen capture streams, a few dozen live hipGraphs in the process) the two streams of the
    # ConvBlock backward no longer overlap and the same training step measures 25.0 ms instead of 22.7 (scripts/bench_order_probe.py;
    # the fit measures the same either way) -- an artefact of doing both in one process, which no deployment does
    # The headline above is measured; the records below are extras of the same line.  Neither a record that throws nor one that
    # never returns (a collective that hangs cannot be interrupted from Python) may cost the line: an exception is recorded in the
    # record's place, and a watchdog sends the line with what is there after CHORE_BENCH_RECORDS_DEADLINE_S (default 900 s; the
    # default N = 1 run needs ~60 s for all of them) and ends the process.
    import threading
    import traceback
    stage = {"name": "", "t0": time.perf_counter()}
    deadline = float(os.environ.get("CHORE_BENCH_RECORDS_DEADLINE_S", "900"))

    def finish(aborted=None):
        if ctx.rank == 0:
            for name, rec in subs.items():
                out[name] = {k: rec[k] for k in rec if k not in ("n_gpus", "data", "scaling", "vs_baseline")} if rec else rec
            if aborted:
                out["records_aborted"] = aborted
        return out

    def bail():
        why = {"stage": stage["name"], "after_s": round(time.perf_counter() - stage["t0"], 1),
               "why": "the record did not return within the deadline; the line carries the headline and the records finished before it"}
        print("[bench] rank %d: records deadline reached in '%s'" % (ctx.rank, stage["name"]), file=sys.stderr, flush=True)
        if ctx.rank == 0 and getattr(ctx, "emit", None):
            ctx.emit(finish(why))
        os._exit(0 if ctx.rank == 0 else 0)
    dog = None
    if deadline > 0:
        dog = threading.Timer(deadline + (0 if ctx.rank == 0 else 10), bail)
        dog.daemon = True
        dog.start()
    for name, fn, over in (("train", mode_train, dict(steps=20, warmup=8, dtype="fp16x3", mode="train", train_other_modes=True)),
                           ("fit", mode_fit, dict(steps=5, warmup=1, dtype="fp16x3", mode="fit")),
                           # configs[4] as BASELINE states it: fp16 fields + hipGraph-captured inner iteration, 8 frames per GPU
                           ("fit_fp16_fields", mode_fit, dict(steps=2, warmup=1, dtype="fp16", mode="fit", frames_per_gpu=8,
                                                              no_cpu_baseline=True))):
        a = copy.copy(args)
        for k, v in over.items():
            setattr(a, k, v)
        if ctx.cuda:
            torch.cuda.empty_cache()
        _stage(ctx, "all: " + name)
        stage["name"] = name
        try:
            subs[name] = fn(a, ctx)
        except Exception as e:
            traceback.print_exc()
            subs[name] = {"error": repr(e)[:400]}
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
    stage["name"] = "query re-timed"
    again = ctx.requery() if getattr(ctx, "requery", None) else None
    if ctx.rank == 0:
        if again is not None:
            alive = bool(ctx.group1 is not None or ctx.world > 1)
            again.update(rccl_communicator_alive=alive, note="the query step re-timed after the training and fit records, in the same process")
            out["with_rccl_communicator"] = again
        finish()
        out["records"] = {"fit": "BASELINE metric 2 (ms per fit iteration), configs[2] / configs[4]: same function as --mode fit, 5 chains after "
                                 "1 warm-up chain (medians per phase in fit.per_phase)", "train": "BASELINE metric 3 (training steps/s), configs[3]: same function as --mode train, "
                                                             "20 steps after 8 warm-up steps, in the fp16x3 mode = the reference's fp32 training "
                                                             "precision on the fp16 matrix cores (round 5); train.other_modes: bf16 (faster, percent-level "
                                                             "gradient error) and fp32 (native fp32 MFMA), each with its measured gradient error",
                          "fit_fp16_fields": "BASELINE configs[4]'s per-GPU share in its stated mode: 8 frames per GPU fitted as one batch on fp16 "
                                             "fields (IEEE half feature maps), every inner iteration a hipGraph replay; 2 chains after 1 warm-up; the "
                                             "mode's field error is other_modes.fp16.field_err"}
    if dog is not None:
        dog.cancel()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--mode", default="all", choices=["all", "query", "fit", "train"])
    ap.add_argument("--dtype", default=None, choices=["bf16", "fp32", "fp16x3", "fp16"],
                    help="default: fp16x3 (fp32-grade: meets the 1e-4 field tolerance; trains at the reference's fp32 precision)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--frames-per-gpu", type=int, default=0, help="fit mode: frames fitted as one batch per GPU (default 1, or 8 when N > 1)")
    ap.add_argument("--eager", action="store_true", help="fit mode: issue the inner iterations from Python instead of replaying hipGraphs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--in-flight", type=int, default=2, help="query mode: recordings of the step replayed round robin on their own streams (1 = one step at a time)")
    ap.add_argument("--eager-step", action="store_true", help="query / train mode: time eager steps instead of hipGraph replays of the step")
    ap.add_argument("--no-ddp", action="store_true", help="N = 1 training record without a process group / gradient reduction (A/B)")
    ap.add_argument("--reducer", default="arena", choices=["arena", "ddp"],
                    help="training: gradient reduction of the primary number (arena = FlatGradReducer, ddp = torch's DistributedDataParallel)")
    ap.add_argument("--reducer-layout", default="auto", choices=["auto", "segmented", "flat"],
                    help="training, arena reducer: segmented = one slice per hourglass stack, all-reduced under the backward (round 5); flat = 4 chunks after it")
    ap.add_argument("--collective", default="all_reduce", choices=["all_reduce", "rs_ag"],
                    help="training, segmented arena: one all_reduce per segment, or reduce_scatter + all_gather")
    ap.add_argument("--train-other-modes", action="store_true", help="train mode: also time the other precision modes and measure every mode's gradient error")
    ap.add_argument("--dry-run", action="store_true", help="launch / rendezvous / timing skeleton only (no GPU needed): CPU + gloo")
    ap.add_argument("--full", action="store_true",
                    help="mode all / query: after the timed steps also measure and check everything else (component and kernel timings, "
                         "roofline, field errors, other precisions, CPU baselines; mode all: the fit and train records)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="mode all / query: write the outputs of the last timed step (df, pca, parts, centers; float32) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.dump_outputs and (args.mode in ("fit", "train") or args.dry_run):
        ap.error("--dump-outputs writes the query step's outputs: --mode all or query, without --dry-run")
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)            # (before fd 1 is redirected: the launched ranks inherit the real stdout)
    # ONE JSON line on stdout, nothing else: C libraries (RCCL prints a version banner) write to file descriptor 1 behind Python's
    # back, so fd 1 is pointed at stderr for the whole run and the line goes to a duplicate of the original stdout
    sys.stdout.flush()
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    defaults = {"all": (20, 5), "query": (20, 5), "fit": (5, 1), "train": (10, 3)}[args.mode]
    if args.dtype is None:
        args.dtype = "fp16x3"
    args.steps = defaults[0] if args.steps is None else args.steps
    args.warmup = defaults[1] if args.warmup is None else args.warmup
    # the one-rank process group is for the training record: --mode train, or --mode all --full
    train_record = args.mode == "train" or (args.mode == "all" and args.full)
    # --dry-run: CPU + gloo even where GPUs are present (N ranks on a box with fewer GPUs)
    ctx = Ctx(args.gpus, one_rank_group=(train_record and not args.dry_run and not args.no_ddp), use_gpu=not args.dry_run)
    if args.dry_run:
        # the distributed skeleton without the device work: used by the CPU test of the N > 1 launch path
        elapsed = ctx.timed(lambda: time.sleep(0.001 * (1 + ctx.rank)), args.steps, args.warmup)
        if ctx.rank == 0:
            line = base_line(args, ctx, "dry run", args.steps / elapsed, "steps/s", elapsed, True, "none",
                             {"workload": "dry run (no device work)"})
            if args.mode == "all" and args.full:    # the shape of the real line: the sub-records and their keys (tests/test_bench_launch.py)
                sub = {"metric": "dry run", "value": 0.0, "unit": "-", "steps": 0, "warmup": 0, "ms_per_step": 0.0,
                       "higher_is_better": True, "dtype": "none", "config": {"workload": "dry run"},
                       "roofline": {"bound": "mfma", "achieved": 0.0, "peak": 1.0, "unit": "TFLOP/s", "frac": 0.0, "traffic": None},
                       "cpu_baseline": {"value": 0.0, "unit": "-", "cores": 0, "kind": "port", "sample": "dry run"}}
                line.update({"roofline": dict(sub["roofline"]), "cpu_baseline": dict(sub["cpu_baseline"]), "fit": dict(sub),
                             "train": dict(sub), "query_fwd_bwd_points_per_s": 0.0})
                if ctx.world > 1:
                    line["train"]["allreduce"] = {"ms_per_step_synced": 0.0, "ms_per_step_no_sync": 0.0, "share_of_step": 0.0}
            emit_line(line, real_stdout)
        ctx.close()
        return
    if not ctx.cuda:
        raise SystemExit("bench.py needs a GPU (there is no CPU path); --dry-run exercises the launch skeleton only")
    ctx.emit = lambda line: emit_line(line, real_stdout)
    out = {"all": mode_all, "query": mode_query, "fit": mode_fit, "train": mode_train}[args.mode](args, ctx)
    ctx.close()
    if ctx.rank == 0:
        emit_line(out, real_stdout)


if __name__ == "__main__":
    main()
