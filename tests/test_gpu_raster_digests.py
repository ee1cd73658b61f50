"""GPU: the bits of the rasteriser family, pinned.  One child process runs every case of tests/raster_digest_cases.py through the
public calls (rasterize_rgbad forward and, through autograd, backward; splat_points; rasterize_scene; rasterize_instances; the
silhouette operator forward and backward) and hands back one sha256 per call; the parent compares them with the digests recorded
before the family's kernels were rebuilt on shared helpers.  A difference means an output bit changed.

    python tests/test_gpu_raster_digests.py --record      prints the DIGESTS table of this build"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_digest_cases as rc      # noqa: E402
from gpu_child import ChildRunner      # noqa: E402

pytestmark = pytest.mark.gpu

RUNNER = ChildRunner(__file__, lambda k: False)


def run_case(kind, p):
    """-> the returned tensors of one call as [(name, numpy array or None)], in a fixed order"""
    import torch
    from chore_amd.render import rasterize_instances, rasterize_rgbad, rasterize_scene, splat_points
    dev = lambda a: None if a is None else torch.as_tensor(a).cuda()      # noqa: E731
    host = lambda t: None if t is None else t.detach().cpu().numpy()      # noqa: E731
    if kind == "silhouette":
        from chore_amd.recon.obj_pose_roi import _RasterizeFn
        tri = dev(rc.triangles(1, p["F"])).requires_grad_(True)
        alpha, fim = _RasterizeFn.apply(tri, p["size"])
        g, = torch.autograd.grad(alpha, tri, dev(rc.upstream(2, p["size"])["alpha"]))
        return [("alpha", host(alpha)), ("face_index", host(fim)), ("grad_faces", host(g))]
    aa = p["ssaa"] == 2
    if kind in ("render", "render_bwd", "scene"):
        tri, tex = dev(rc.triangles(3, p["F"])), dev(rc.textures(4, p["F"], p.get("ts", 2)))
        lt = dev(rc.light(5, p["F"])) if p.get("lit", True) else None
    if kind == "render":
        out = rasterize_rgbad(tri, tex, lt, p["size"], aa, rc.NEAR, rc.FAR, return_index=True)
        return [(k, host(out[k])) for k in ("rgb", "depth", "alpha", "face_index")]
    if kind == "render_bwd":
        leaves = [x.requires_grad_(True) for x in (tri, tex, lt) if x is not None]
        out = rasterize_rgbad(tri, tex, lt, p["size"], aa, rc.NEAR, rc.FAR, return_index=True)
        up = rc.upstream(6, p["size"])
        given = p["up"].split("+")
        grads = torch.autograd.grad([out[k] for k in given], leaves, [dev(up[k]) for k in given], allow_unused=True)
        grads = list(grads) + [None] * (3 - len(grads))
        return [(k, host(out[k])) for k in ("rgb", "depth", "alpha", "face_index")] + \
               [(k, host(g)) for k, g in zip(("grad_faces", "grad_textures", "grad_light"), grads)]
    if kind in ("splat", "scene"):
        pts, col, rad = rc.points(7)
    if kind == "splat":
        out = splat_points(dev(pts), dev(col) if p["colored"] else None, dev(rad) if p["per_point"] else 1.5, p["size"], aa, rc.NEAR,
                           rc.FAR, background_color=(0.1, 0.2, 0.3), return_index=True)
        return [(k, host(out[k])) for k in ("rgb", "depth", "alpha", "point_index")]
    if kind == "scene":
        grp = dev(rc.face_group(8, p["F"], 4)) if p["grouped"] else None
        op = dev(rc.face_opacity(9, p["F"])) if p["opacity"] else None
        out = rasterize_scene(tri, tex, lt, dev(pts), dev(col), dev(rad), op, p["bias"], p["size"], aa, rc.NEAR, rc.FAR,
                              background_color=(0.1, 0.2, 0.3), return_index=True, face_layers=p["layers"], face_group=grp)
        return [(k, host(out[k])) for k in ("rgb", "depth", "alpha", "sample_id")]
    if kind == "instances":
        out = rasterize_instances(dev(rc.triangles(3, p["F"])), dev(rc.face_group(10, p["F"], p["G"] + 1)), p["G"], p["size"], aa,
                                  rc.NEAR, rc.FAR, return_index=True)
        return [(k, host(out[k])) for k in ("visible", "full", "face_samples", "group_samples", "face_index")]
    raise ValueError(kind)


def digests_of(ids):
    return [rc.digest(run_case(rc.CASES[cid][1], rc.CASES[cid][2])) for cid in ids]


def test_digests(tmp_path):
    ids = sorted(rc.CASES)
    out, path = RUNNER.run(tmp_path, "digests", {}, {}, ids, 120)
    try:
        got = dict(zip(ids, (str(d) for d in out["digests"])))
    finally:
        out.close()
        os.remove(path)
    bad = [cid for cid in ids if got[cid] != rc.DIGESTS[cid]]
    for cid in bad:
        print("  %-60s recorded %s, now %s" % (cid, rc.DIGESTS[cid][:16], got[cid][:16]))
    assert not bad, "%d of %d calls changed a bit: %s" % (len(bad), len(ids), bad)


if __name__ == "__main__":
    import json
    if sys.argv[1] == "--child":
        with open(sys.argv[3]) as f:
            jobs = json.load(f)
        np.savez(sys.argv[4], digests=np.asarray(digests_of(jobs)))
    elif sys.argv[1] == "--record":
        for cid, d in zip(sorted(rc.CASES), digests_of(sorted(rc.CASES))):
            print('    "%s": "%s",' % (cid, d))
