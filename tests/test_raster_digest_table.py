"""CPU: what tests/test_gpu_raster_digests.py covers, checked without a GPU.
  * every entry point the six rasteriser files export (csrc/silhouette.hip, render.hip, render_bwd.hip, splat.hip, scene.hip,
    instances.hip) has at least one case in raster_digest_cases.py; the two projection entry points of silhouette.hip launch no
    kernel of the family and are named as left out;
  * the case file carries exactly one sha256 per case;
  * the inputs are what the cases say: front-facing or zero-area triangles over one tile, the zero-area triangle and the depth
    tie, radii on both sides of two samples at both sample counts, the clamped radius and the four border points."""
import os
import re

import numpy as np

import raster_digest_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("silhouette.hip", "render.hip", "render_bwd.hip", "splat.hip", "scene.hip", "instances.hip")
NOT_RASTERISERS = {"chore_sil_project_fwd", "chore_sil_project_bwd"}      # placement and camera projection of the template


def test_every_entry_point_has_a_case():
    exported = set()
    for f in FILES:
        exported |= set(re.findall(r'extern "C" int (chore_\w+)\(', open(os.path.join(REPO, "chore_amd", "csrc", f)).read()))
    assert exported - NOT_RASTERISERS == set(rc.ENTRY_POINTS), sorted(exported ^ set(rc.ENTRY_POINTS))
    count = {e: sum(e in entries for entries, _, _ in rc.CASES.values()) for e in rc.ENTRY_POINTS}
    print("cases per entry point:", count)
    assert all(count.values()), count
    assert {e for entries, _, _ in rc.CASES.values() for e in entries} <= set(rc.ENTRY_POINTS)


def test_one_digest_per_case():
    assert set(rc.DIGESTS) == set(rc.CASES)
    assert all(re.fullmatch(r"[0-9a-f]{64}", d) for d in rc.DIGESTS.values())
    assert len(set(rc.DIGESTS.values())) == len(rc.DIGESTS)               # no two calls return the same bits


def test_inputs_are_what_the_cases_say():
    for F in (257, 600):
        t = rc.triangles(3, F)
        f = t.reshape(rc.B, F, 9)
        a, b = (f[..., 7] - f[..., 1]) * (f[..., 3] - f[..., 0]), (f[..., 4] - f[..., 1]) * (f[..., 6] - f[..., 0])
        assert t.dtype == np.float32 and not (a < b).any()                # nothing is culled: the bin's list holds all F
        assert (a[:, 5] == b[:, 5]).all() and np.array_equal(t[:, 9], t[:, 2])
        px = 0.5 * ((t[:, :F - 1, 0, :2] * 136 + 136) - 1)                # first vertices inside tile 1 of a 136-pixel image
        assert (px > 16).all() and (px < 31).all()
    _, _, rad = rc.points(7)
    for ss in (1, 2):
        assert (rad[:, 5:] * ss <= 2).any() and (rad[:, 5:] * ss > 2).any()
    assert (rad[:, 0] * 1 > 64).all() and (rad[:, 1:5] == 3).all()
    sizes = {p["size"] for _, _, p in rc.CASES.values()}
    assert sizes == {33, 64, 136} and {p["F"] for _, _, p in rc.CASES.values() if "F" in p} == {257, 600}
    scene = [p for _, k, p in rc.CASES.values() if k == "scene"]
    assert {p["layers"] for p in scene} == {1, 2, 3, 8} and {p["bias"] for p in scene} == {0.0, 0.25}
    assert {(p["grouped"], p["opacity"]) for p in scene} == {(False, False), (False, True), (True, False), (True, True)}
    ups = {p["up"] for _, k, p in rc.CASES.values() if k == "render_bwd"}
    assert ups == {"rgb+depth+alpha", "rgb", "depth", "alpha"}
