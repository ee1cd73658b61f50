"""The cases and the recorded bits of tests/test_gpu_raster_digests.py: every entry point of the rasteriser family (silhouette,
render forward and backward, splat, scene, scene layers, instances) on inputs built on the host from numpy.random.RandomState
seeds, and one sha256 per call over all returned tensors in a fixed order.  The digests were recorded on an MI355X at the commit
BEFORE the family's shared helpers were introduced (18b902a) and pin its bits across that refactor and every later one: a kernel
of the family may change its code, never a bit of its output.  All calls take PROJECTED triangles and points, so no torch
arithmetic lies between these arrays and the kernels.  No torch import here: tests/test_raster_digest_table.py reads this file
without a GPU.

The shapes are the smallest that reach every shared piece: image sizes 33 (a tile tail) and 136 (at ssaa 2: 272 samples, two bins
per axis); B = 2; F = 257 and 600 with every triangle's box over one tile of one bin, so that tile's hit list crosses the 256-entry
chunk; one zero-area triangle and one exact depth tie; texture sizes 2 and 4 with and without light; points with a scalar radius
and with per-point radii on both sides of 2 samples, one clamped at 64 samples and one overhanging each border."""
import hashlib

import numpy as np

NEAR, FAR = 0.1, 100.0
B = 2
ENTRY_POINTS = ("chore_silhouette_fwd", "chore_silhouette_bwd", "chore_render_fwd", "chore_render_bwd", "chore_splat_fwd",
                "chore_scene_fwd", "chore_scene_layers_fwd", "chore_instances_fwd")


def triangles(seed, F):
    """(B,F,3,3) float32 projected triangles, all front-facing or of zero area.  All but the last have their first vertex inside
    pixels 17..29 of a 136-pixel image (tile 1 of bin 0 at both sample counts; tile 0 at size 33) and the others within 0.5 of it;
    the last spans the view, so the other bins are not empty.  Triangle 5 has zero area, triangle 9 is triangle 2 again (an
    exact depth tie, decided by the index)."""
    rs = np.random.RandomState(seed)
    v0 = rs.uniform(-0.74, -0.56, (B, F, 1, 2))
    xy = np.concatenate([v0, v0 + rs.uniform(-0.5, 0.5, (B, F, 2, 2))], 2)
    t = np.concatenate([xy, rs.uniform(0.5, 4.0, (B, F, 3, 1))], 3).astype(np.float32)
    t[:, F - 1, :, :2] = np.float32([[-1.1, -1.05], [1.15, -0.9], [0.1, 1.2]])
    t[:, 5, :, :2] = np.float32([[-0.625, -0.625], [-0.5, -0.5625], [-0.375, -0.5]])
    f = t.reshape(B, F, 9)
    back = (f[..., 7] - f[..., 1]) * (f[..., 3] - f[..., 0]) < (f[..., 4] - f[..., 1]) * (f[..., 6] - f[..., 0])     # tri_backside
    t[back] = t[back][:, [0, 2, 1]]
    t[:, 9] = t[:, 2]
    return t


def textures(seed, F, ts):
    return np.random.RandomState(seed).uniform(0.0, 1.0, (B, F, ts, ts, ts, 3)).astype(np.float32)


def light(seed, F):
    return np.random.RandomState(seed).uniform(0.2, 1.2, (B, F, 3)).astype(np.float32)


def points(seed, N=300):
    """(B,N,3) points over the view and a little outside, their colours, and per-point radii (output pixels) between 0.3 and 3:
    on both sides of 2 samples at both sample counts.  Point 0 asks for 100 pixels (clamped at 64 samples); points 1..4 sit
    on the four borders with 3 pixels, overhanging them."""
    rs = np.random.RandomState(seed)
    p = np.concatenate([rs.uniform(-1.05, 1.05, (B, N, 2)), rs.uniform(0.5, 4.0, (B, N, 1))], 2).astype(np.float32)
    col = rs.uniform(0.0, 1.0, (B, N, 3)).astype(np.float32)
    rad = rs.uniform(0.3, 3.0, (B, N)).astype(np.float32)
    p[:, 0, :2], rad[:, 0] = np.float32([0.3, -0.2]), 100.0
    p[:, 1:5, :2] = np.float32([[-1.0, 0.1], [1.0, -0.3], [0.2, -1.0], [-0.4, 1.0]])
    rad[:, 1:5] = 3.0
    return p, col, rad


def upstream(seed, size):
    rs = np.random.RandomState(seed)
    return {"rgb": rs.standard_normal((B, 3, size, size)).astype(np.float32),
            "depth": rs.standard_normal((B, size, size)).astype(np.float32),
            "alpha": rs.standard_normal((B, size, size)).astype(np.float32)}


def face_group(seed, F, n):
    return np.random.RandomState(seed).randint(0, n, (B, F)).astype(np.int32)


def face_opacity(seed, F):
    """a third opaque, the rest in [0, 1)"""
    rs = np.random.RandomState(seed)
    o = rs.uniform(0.0, 1.0, (B, F)).astype(np.float32)
    o[rs.uniform(size=(B, F)) < 0.33] = 1.0
    return o


# id -> (entry points the call reaches, kind, parameters).  The seed of every input follows from the parameters alone.
CASES = {}


def _add(cid, entries, kind, **kw):
    assert cid not in CASES
    CASES[cid] = (entries, kind, kw)


for _size in (33, 64):
    _add("sil_%d" % _size, ("chore_silhouette_fwd", "chore_silhouette_bwd"), "silhouette", size=_size, F=257)
for _size, _ssaa, _F, _ts, _lt in ((33, 1, 257, 2, False), (33, 2, 600, 4, True), (136, 1, 600, 2, True), (136, 2, 257, 4, False)):
    _add("render_%d_x%d_F%d_ts%d_%s" % (_size, _ssaa, _F, _ts, "lit" if _lt else "unlit"), ("chore_render_fwd",), "render",
         size=_size, ssaa=_ssaa, F=_F, ts=_ts, lit=_lt)
for _size, _ssaa, _F, _ts, _lt, _up in ((33, 2, 257, 2, True, "rgb+depth+alpha"), (136, 2, 600, 4, True, "rgb+depth+alpha"),
                                        (33, 1, 257, 4, False, "rgb"), (136, 1, 257, 2, True, "depth"), (33, 2, 600, 2, True, "alpha"),
                                        (136, 2, 257, 2, False, "rgb")):
    _add("render_bwd_%d_x%d_F%d_ts%d_%s_%s" % (_size, _ssaa, _F, _ts, "lit" if _lt else "unlit", _up),
         ("chore_render_fwd", "chore_render_bwd"), "render_bwd", size=_size, ssaa=_ssaa, F=_F, ts=_ts, lit=_lt, up=_up)
for _size, _ssaa, _per, _col in ((33, 1, False, True), (33, 2, False, False), (136, 1, True, True), (136, 2, True, True)):
    _add("splat_%d_x%d_%s_%s" % (_size, _ssaa, "radii" if _per else "r1.5", "col" if _col else "white"), ("chore_splat_fwd",), "splat",
         size=_size, ssaa=_ssaa, per_point=_per, colored=_col)
for _layers, _grp, _op, _bias, _size, _ssaa, _F in ((1, False, False, 0.0, 33, 1, 257), (1, False, True, 0.25, 136, 2, 600),
                                                    (1, True, True, 0.0, 33, 2, 257), (2, True, True, 0.0, 136, 1, 600),
                                                    (2, False, False, 0.25, 33, 2, 257), (3, True, False, 0.25, 136, 2, 257),
                                                    (3, False, True, 0.0, 33, 1, 600), (8, True, True, 0.25, 33, 2, 600),
                                                    (8, False, False, 0.0, 136, 2, 257), (8, False, True, 0.25, 33, 1, 257)):
    _add("scene_L%d_%s_%s_b%g_%d_x%d_F%d" % (_layers, "grp" if _grp else "nogrp", "op" if _op else "opaque", _bias, _size, _ssaa, _F),
         ("chore_scene_fwd",) if _layers == 1 and not _grp else ("chore_scene_layers_fwd",), "scene", layers=_layers, grouped=_grp,
         opacity=_op, bias=_bias, size=_size, ssaa=_ssaa, F=_F)
for _G, _size, _ssaa, _F in ((1, 33, 2, 257), (3, 136, 2, 600), (3, 33, 1, 257), (1, 136, 1, 600)):
    _add("instances_G%d_%d_x%d_F%d" % (_G, _size, _ssaa, _F), ("chore_instances_fwd",), "instances", G=_G, size=_size, ssaa=_ssaa, F=_F)


def digest(named):
    """sha256 over (name, dtype, shape, bytes) of every returned array, in the order given; None = an absent output"""
    h = hashlib.sha256()
    for name, a in named:
        if a is None:
            h.update(("%s:none;" % name).encode())
            continue
        a = np.ascontiguousarray(a)
        h.update(("%s:%s:%s;" % (name, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# recorded on an MI355X at 18b902a (two processes, equal), one per case
DIGESTS = {
    "instances_G1_136_x1_F600": "a3bab5dd6c84a5b244c85682250a1831ef9d667b2238da6eb2ed942975ca758d",
    "instances_G1_33_x2_F257": "95b60ba8a4073e39aeff11631152e5f57c8e1cb544adf8988c1180148da74e14",
    "instances_G3_136_x2_F600": "3538ca0ac7ae5a5836aab2cae7239c2c5521f406c9f78817a9b51ed8e3450f29",
    "instances_G3_33_x1_F257": "ed76562ae9b1a21cc357b966d0a00ff707af08bb5242272e461d2769c2d8a747",
    "render_136_x1_F600_ts2_lit": "d4f1897cb11fe9302d5ef0b85297ef73748a6d2b307a1abbbf8c6b023b962ab2",
    "render_136_x2_F257_ts4_unlit": "b813e3e1b69e1afd5ddd015f3ed4dbec9e2d641987bf41a3c03888b4b63f5aa7",
    "render_33_x1_F257_ts2_unlit": "e75ee63601870e5970768988eb3311683c6b4d61a3d759b2ff971dd942d438aa",
    "render_33_x2_F600_ts4_lit": "f83c9e65cf873e856e51aa547512029b61f8ea3fa563cc3705d52d3f35c76ef0",
    "render_bwd_136_x1_F257_ts2_lit_depth": "360e688cb27a8d31054ffd6ea1ae63f245ae7815fb347e7a3290031aeb9e8254",
    "render_bwd_136_x2_F257_ts2_unlit_rgb": "1dc5d622cc0aca94ee23106d5d197f4073583b173f03c8034cca7c13ef00e8b5",
    "render_bwd_136_x2_F600_ts4_lit_rgb+depth+alpha": "8f1ee5351ab3c445275e2e8b5664ea25b53527889be3e2fe145651aeb57a0c8d",
    "render_bwd_33_x1_F257_ts4_unlit_rgb": "a02d0f571bf955cc1bb6cb5b65d4b0ca3747064cf85903123bb03374dc5f8a1e",
    "render_bwd_33_x2_F257_ts2_lit_rgb+depth+alpha": "1aacc8dc3713d40a4a5a2ab6d576144bc8248200af210a5a5117313c88eae5f5",
    "render_bwd_33_x2_F600_ts2_lit_alpha": "3b9e914d36e6344bc2756ee575b7b9aea961bb4ea3af8815baa5efd5cb0f66ae",
    "scene_L1_grp_op_b0_33_x2_F257": "f594c2ab2eb69cc14a6b10cd3080b34af2dd8d3db96698a1bdc2f00865419574",
    "scene_L1_nogrp_op_b0.25_136_x2_F600": "f2a8bac618f912813b6263431b92a400079d80db8c276318ed562cad3406d6f1",
    "scene_L1_nogrp_opaque_b0_33_x1_F257": "736cb2a3917e09c0fbe2e586ba13ada8b19008a1a856c191d3d62f3119e0f001",
    "scene_L2_grp_op_b0_136_x1_F600": "1286cdaa64b3eb13b28c10e0a6e9e1fbd21a8e3a8d07263f4a85b1d1e0f4b18a",
    "scene_L2_nogrp_opaque_b0.25_33_x2_F257": "b2664cfdd16662d4c12a171f07cffa9e3fa73d82f9e06c4d710dff3f3de9b2e0",
    "scene_L3_grp_opaque_b0.25_136_x2_F257": "8f0d2c269e93ae0962824b82df202298b791ff6bdc79476824d9c6f9204faaa4",
    "scene_L3_nogrp_op_b0_33_x1_F600": "35770f78a4c5e4ec11161fbff998a63e744b61f54070bee96b938d9ff8f43671",
    "scene_L8_grp_op_b0.25_33_x2_F600": "70126046e82d897906e897aba74f9a91e0df012d54146df4a8ac4259dd82caa4",
    "scene_L8_nogrp_op_b0.25_33_x1_F257": "1737ebaf5451294de104f9460c5488873001130b6eba1c583c84be4e536fe03f",
    "scene_L8_nogrp_opaque_b0_136_x2_F257": "e4c71dcc0445fc778f578fcbd8682c44a994f9c78274664f29447869812cb7d0",
    "sil_33": "bcdbf542ccbbad0ce3bbf375e802d6a7f6a83b7999e5dc162cc3123a942ea65f",
    "sil_64": "af5af354813692e333d505f7cab9ed79624f8700023854b57d159d480ec792c2",
    "splat_136_x1_radii_col": "6a0ebf441429677bda03f9b0a39609f2d7ffe411c12a19294fe99b2ed75d17c1",
    "splat_136_x2_radii_col": "916a724ffd822d3a8247973a2ded99a2eb78795b2505a577268ee440c55e9f04",
    "splat_33_x1_r1.5_col": "2edda58193a271ba73349a340604aa87550e0876ef7ce8a0cbd566b346f3afb7",
    "splat_33_x2_r1.5_white": "d74604faae563a75e7f6730255d9b6f523a7828732a260f9b43aa83cc70d08a9",
}
