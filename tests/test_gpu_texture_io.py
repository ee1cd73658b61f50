"""GPU: textured OBJ files (csrc/texture_io.hip: chore_load_textures, chore_texture_atlas; chore_amd.render.obj_io) against the
float64 restatement tests/texture_io_ref.py, at the smallest shapes where the kernels can go wrong; the round trip through the
files; and the fitter's EXPORT_TEXTURED_OBJ on the two-frame synthetic fit of tests/test_gpu_fit_debug.py.

Worst figures the tests printed on an MI355X: load, bilinear 6.5e-6 (tolerance 1e-4), nearest exact outside a left-out set of at
most 0.34 % of a case (cap 2 %); atlas 1.6e-7 (tolerance 2e-5); round trip, constant colours 6.9e-6 (bound 1e-4) and the corner
texels of random cubes 1.97e-3 (bound 0.5 / 255 + 5e-4 = 2.46e-3)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import png_ref
import texture_io_ref as tref

pytestmark = pytest.mark.gpu

EINVAL = -1


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def hip_load(uv, face_image, face_color, images, ts, wrap, bilinear):
    from chore_amd.render import obj_io
    tex = obj_io.sample_textures(uv, face_image, face_color, images, ts, wrap, bilinear)
    assert tex.shape == (len(uv), ts, ts, ts, 3) and tex.dtype == torch.float32 and tex.is_cuda
    return tex.cpu().numpy()


# ---- 1. load against the restatement ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bilinear", [True, False])
@pytest.mark.parametrize("wrap", sorted(tref.UV_RANGE))
@pytest.mark.parametrize("F,ts,H,W", tref.LOAD_CASES)
def test_load_against_the_restatement(F, ts, H, W, wrap, bilinear):
    uv, fi, fc, images = tref.load_inputs(F, ts, H, W, wrap)
    ref = tref.load_textures(uv, fi, fc, images, ts, tref.WRAPS[wrap], bilinear)
    got = hip_load(uv, fi, fc, images, ts, wrap, bilinear)
    err = np.abs(got - ref["textures"]).max(-1)
    keep = ~ref["left_out"]
    share = float(ref["left_out"].mean())
    print("F=%d ts=%d %dx%d %s %s: left out %.4f, worst error %.3g (left-out texels: %.3g)"
          % (F, ts, H, W, wrap, "bilinear" if bilinear else "nearest", share, err[keep].max(),
             err[~keep].max() if (~keep).any() else 0))
    assert share <= tref.LEFT_OUT_CAP
    if bilinear:
        assert not ref["left_out"].any()
        assert err.max() <= tref.LOAD_TOL
    else:
        assert np.array_equal(got[keep], ref["textures"][keep].astype(np.float32))
    colour_only = fi < 0
    assert np.array_equal(got[colour_only], np.broadcast_to(fc[colour_only, None, None, None, :], got[colour_only].shape))


# ---- 2. load, exact -------------------------------------------------------------------------------------------------

def test_load_exact_values():
    rng = np.random.default_rng(5)
    F, ts = 37, 4
    uv = rng.uniform(-2.5, 3.5, (F, 3, 2)).astype(np.float32)
    fc = rng.uniform(0, 1, (F, 3)).astype(np.float32)
    fi = np.asarray([(0, 0, -1)[f % 3] for f in range(F)], np.int32)
    const = np.empty((5, 9, 3), np.uint8)
    const[:] = (7, 130, 255)
    want = (np.float32([7, 130, 255]) / np.float32(255.0))
    for wrap in ("REPEAT", "MIRRORED_REPEAT", "CLAMP_TO_EDGE"):
        for bilinear in (True, False):
            got = hip_load(uv, fi, fc, [const], ts, wrap, bilinear)
            assert np.array_equal(got[fi == 0], np.broadcast_to(want, got[fi == 0].shape)), (wrap, bilinear)   # a constant image: u8 / 255
            assert np.array_equal(got[fi < 0], np.broadcast_to(fc[fi < 0, None, None, None, :], got[fi < 0].shape))
    # CLAMP_TO_BORDER: zeros on every textured face, never sampled
    got = hip_load(uv, fi, fc, [const], ts, "CLAMP_TO_BORDER", True)
    assert not got[fi == 0].any() and np.array_equal(got[fi < 0], np.broadcast_to(fc[fi < 0, None, None, None, :], got[fi < 0].shape))
    # an index past the table and a non-finite coordinate: the face's colour
    uv_bad = uv.copy()
    uv_bad[0, 1, 0], uv_bad[1, 2, 1] = np.nan, np.inf
    got = hip_load(uv_bad, np.where(np.arange(F) == 2, 5, fi).astype(np.int32), fc, [const], ts, "REPEAT", True)
    for f in (0, 1, 2):
        assert np.array_equal(got[f], np.broadcast_to(fc[f], got[f].shape)), f


@pytest.mark.parametrize("bilinear", [True, False])
def test_load_pixel_centres(bilinear):
    """W-1 and H-1 powers of two and UVs on pixel centres: the three one-hot texels of a face are its pixels exactly, and texel
    (0,0,0) is flipped pixel (0,0)"""
    rng = np.random.default_rng(6)
    F, ts, H, W = 20, 3, 9, 17
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    px = np.stack([rng.integers(0, W, (F, 3)), rng.integers(0, H, (F, 3))], -1)
    uv = (px / np.float64([W - 1, H - 1])).astype(np.float32)            # exact: multiples of 1/16 and 1/8
    fc = np.zeros((F, 3), np.float32)
    flipped = img[::-1].astype(np.float32) / np.float32(255.0)
    got = hip_load(uv, np.zeros(F, np.int32), fc, [img], ts, "CLAMP_TO_EDGE", bilinear)
    for c, idx in enumerate(((ts - 1, 0, 0), (0, ts - 1, 0), (0, 0, ts - 1))):
        assert np.array_equal(got[(slice(None),) + idx], flipped[px[:, c, 1], px[:, c, 0]]), c
    assert np.array_equal(got[:, 0, 0, 0], np.broadcast_to(flipped[0, 0], (F, 3)))


def test_load_twice_bit_equal():
    F, ts, H, W = tref.LOAD_CASES[-1]
    uv, fi, fc, images = tref.load_inputs(F, ts, H, W, "MIRRORED_REPEAT")
    a = hip_load(uv, fi, fc, images, ts, "MIRRORED_REPEAT", True)
    b = hip_load(uv, fi, fc, images, ts, "MIRRORED_REPEAT", True)
    assert np.array_equal(a, b)


def test_load_refusals_leave_the_output_untouched():
    from chore_amd import _lib
    h = _lib.handle(0)
    F, ts = 3, 2
    uv, fi, fc = dev(np.zeros((F, 3, 2))), dev(np.zeros(F), torch.int32), dev(np.zeros((F, 3)))
    img = dev(np.zeros(2 * 2 * 3), torch.uint8)
    out = torch.full((F, ts, ts, ts, 3), -7.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(uv_p=uv.data_ptr(), fi_p=fi.data_ptr(), fc_p=fc.data_ptr(), img_p=img.data_ptr(), nbytes=12, off=(0,), hw=(2, 2), M=1,
             F=F, ts=ts, wrapping=0, out_p=out.data_ptr(), off_null=False, hw_null=False):
        off_c = None if off_null else (ctypes.c_int64 * len(off))(*off)
        hw_c = None if hw_null else (ctypes.c_int * len(hw))(*hw)
        return _lib.lib.chore_load_textures(h, uv_p, fi_p, fc_p, img_p, nbytes, off_c, hw_c, M, F, ts, wrapping, 1, out_p, stream)
    bad = [dict(uv_p=None), dict(fi_p=None), dict(fc_p=None), dict(out_p=None), dict(img_p=None), dict(off_null=True),
           dict(hw_null=True), dict(F=0), dict(ts=1), dict(ts=17), dict(M=-1), dict(M=129), dict(hw=(0, 2)), dict(hw=(2, 0)),
           dict(wrapping=4), dict(wrapping=-1), dict(nbytes=11), dict(off=(1,)), dict(off=(-1,))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert _lib.lib.chore_last_error(h)
    assert _lib.lib.chore_load_textures(None, uv.data_ptr(), fi.data_ptr(), fc.data_ptr(), img.data_ptr(), 12,
                                        (ctypes.c_int64 * 1)(0), (ctypes.c_int * 2)(2, 2), 1, F, ts, 0, 1, out.data_ptr(),
                                        stream) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call() == 0 and call(M=0, img_p=None, off_null=True, hw_null=True) == 0         # no images at all is a valid call
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())
    # the atlas' refusals
    tex = torch.zeros(2, 2, 2, 2, 3, device="cuda")
    image = torch.full((16, 32, 3), -7.0, device="cuda")
    for args in ((None, 2, 2, 16, image.data_ptr()), (tex.data_ptr(), 2, 2, 16, None), (tex.data_ptr(), 0, 2, 16, image.data_ptr()),
                 (tex.data_ptr(), 2, 1, 16, image.data_ptr()), (tex.data_ptr(), 2, 17, 16, image.data_ptr()),
                 (tex.data_ptr(), 2, 2, 1, image.data_ptr()), (tex.data_ptr(), 2, 2, 16385, image.data_ptr()),
                 (tex.data_ptr(), 1025 ** 2, 2, 16, image.data_ptr())):
        assert _lib.lib.chore_texture_atlas(h, *args, stream) == EINVAL, args
    torch.cuda.synchronize()
    assert bool((image == -7.0).all())


# ---- 3. atlas against the restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("tso", tref.ATLAS_TSO)
@pytest.mark.parametrize("tsi", tref.ATLAS_TSI)
@pytest.mark.parametrize("F", tref.ATLAS_F)
def test_atlas_against_the_restatement(F, tsi, tso):
    from chore_amd.render import create_texture_image, obj_io
    rng = np.random.default_rng(100 * F + 10 * tsi + tso)
    cubes = rng.uniform(0.05, 1, (F, tsi, tsi, tsi, 3)).astype(np.float32)
    tex = torch.from_numpy(cubes).cuda().clone()                          # exactly F cubes: nothing behind the last one
    assert tex.numel() == F * tsi ** 3 * 3
    ref = tref.texture_atlas(cubes, tso)
    image, vt = create_texture_image(tex, tso)
    tile_w, tile_h = tref.atlas_tiles(F)
    assert image.shape == (tile_h * tso, tile_w * tso, 3) == ref.shape and image.dtype == np.float32
    assert np.array_equal(vt, obj_io.atlas_vertices(F, tso))
    err = np.abs(image - ref).max()
    print("F=%d tsi=%d tso=%d: worst error %.3g" % (F, tsi, tso, err))
    assert err <= tref.ATLAS_TOL
    up = image[::-1]                                                      # rows counted from the bottom
    for fn in range(tile_w * tile_h):
        tile = up[(fn // tile_w) * tso:(fn // tile_w + 1) * tso, (fn % tile_w) * tso:(fn % tile_w + 1) * tso]
        if fn >= F:
            assert not tile.any(), fn                                     # a tile without a face: exactly 0
        else:
            assert tile.min() > 0
            for ly in range(tso - 1):                                     # the diagonal's right neighbour: its left neighbour, bit for bit
                assert np.array_equal(tile[ly, ly + 1], tile[ly, ly]), (fn, ly)
    again, _ = create_texture_image(tex, tso)
    assert np.array_equal(image, again)


# ---- 4. round trip through the files -------------------------------------------------------------------------------------

@pytest.mark.parametrize("F,ts", [(1, 2), (5, 4), (10, 4), (37, 3)])
def test_round_trip_through_the_files(tmp_path, F, ts):
    from chore_amd.render import load_obj, save_obj
    rng = np.random.default_rng(F)
    verts = rng.normal(size=(F + 2, 3)).astype(np.float32)
    faces = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], 1).astype(np.int32)
    printed = np.float32([[float("%.8f" % c) for c in v] for v in verts])
    tile_w, _ = tref.atlas_tiles(F)

    def trip(cubes, name, wrap="CLAMP_TO_EDGE"):
        path = str(tmp_path / name)
        save_obj(path, dev(verts), dev(faces, torch.int32), dev(cubes))
        v, f, t = load_obj(path, normalization=False, load_texture=True, texture_size=ts, texture_wrapping=wrap)
        assert v.is_cuda and f.is_cuda and t.is_cuda and f.dtype == torch.int32 and v.dtype == torch.float32
        assert np.array_equal(v.cpu().numpy(), printed) and np.array_equal(f.cpu().numpy(), faces)
        assert t.shape == (F, ts, ts, ts, 3)
        return t.cpu().numpy()
    # per-face constant colours on the 1/255 grid
    colours = (rng.integers(0, 256, (F, 3)) / 255.0).astype(np.float32)
    const = np.broadcast_to(colours[:, None, None, None, :], (F, ts, ts, ts, 3)).copy()
    back = clamped = trip(const, "const.obj")
    # texel (0,0,0) has three zero weights and samples position (0,0) whatever the face: the corner of face 0's tile
    want = const.copy()
    want[:, 0, 0, 0] = colours[0]
    print("F=%d ts=%d constant colours: worst error %.3g" % (F, ts, np.abs(back - want).max()))
    assert np.abs(back - want).max() <= 1e-4
    # random cubes: the three one-hot corner texels
    cubes = rng.uniform(0, 1, (F, ts, ts, ts, 3)).astype(np.float32)
    back = trip(cubes, "random.obj")
    corners = ((ts - 1, 0, 0), (0, ts - 1, 0), (0, 0, ts - 1))
    worst = max(np.abs(back[(slice(None),) + c] - cubes[(slice(None),) + c]).max() for c in corners)
    print("F=%d ts=%d random cubes: worst corner error %.3g" % (F, ts, worst))
    assert worst <= 0.5 / 255 + 5e-4
    # the reference's REPEAT sends u = 0 to 1: the faces of tile column 0 come back from the wrong end of the atlas
    if F > 1:
        repeat = trip(const, "const.obj", "REPEAT")
        column0 = np.arange(F) % tile_w == 0
        differs = np.abs(repeat - clamped).reshape(F, -1).max(1) > 1e-3
        assert differs[column0].all(), differs
    with pytest.raises(Exception, match="Failed to load textures"):
        path = str(tmp_path / "bare.obj")
        save_obj(path, dev(verts), dev(faces, torch.int32))
        load_obj(path, load_texture=True)
    v, f = load_obj(str(tmp_path / "bare.obj"))                           # normalised into [-1,1]^3 by the reference's four steps
    want = torch.from_numpy(printed).cuda()
    want -= want.min(0)[0][None, :]
    want /= torch.abs(want).max()
    want *= 2
    want -= want.max(0)[0][None, :] / 2
    assert torch.equal(v, want) and np.array_equal(f.cpu().numpy(), faces)


# ---- 5. the fitter ------------------------------------------------------------------------------------------------------

def test_fitter_exports_textured_obj(opt, tmp_path, monkeypatch):
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    from chore_amd.render import load_obj, obj_io
    from chore_amd.recon.assets import read_ply
    from test_gpu_fit_debug import FITTED, _run
    assert ReconFitterBase.EXPORT_TEXTURED_OBJ is False
    plain_dir, export_dir = str(tmp_path / "plain"), str(tmp_path / "export")
    plain, _ = _run(opt, plain_dir, False, False)
    monkeypatch.setattr(ReconFitterBase, "EXPORT_TEXTURED_OBJ", True)
    export, _ = _run(opt, export_dir, False, False)
    for i, (a, b) in enumerate(zip(plain, export)):
        for k in FITTED:
            assert torch.isfinite(a[k]).all(), (i, k)
            assert torch.equal(a[k], b[k]), (i, k, float((a[k] - b[k]).abs().max()))
    for i in range(2):
        sub = os.path.join(f"seq{10 + i}", "t0000.000", "test")
        for what in ("smpl", "object"):
            ply = os.path.join(export_dir, sub, f"k1.{what}.ply")
            assert open(ply, "rb").read() == open(os.path.join(plain_dir, sub, f"k1.{what}.ply"), "rb").read(), (i, what)
            for ext in ("obj", "mtl", "png"):
                assert os.path.exists(os.path.join(export_dir, sub, f"k1.{what}.{ext}")), (i, what, ext)
                assert not os.path.exists(os.path.join(plain_dir, sub, f"k1.{what}.{ext}")), (i, what, ext)
            pv, pf = read_ply(ply)
            name = os.path.join(export_dir, sub, f"k1.{what}.obj")
            v, f, t = load_obj(name, normalization=False, load_texture=True, texture_wrapping="CLAMP_TO_EDGE")
            if what == "smpl":
                assert v.shape == (6890, 3) and f.shape == (13776, 3)
            assert np.array_equal(f.cpu().numpy(), np.asarray(pf)) and t.shape == (len(pf), 4, 4, 4, 3)
            assert np.abs(v.cpu().numpy() - np.asarray(pv, np.float32)).max() <= 1e-8 + 1e-6      # %.8f of the PLY's vertices
            parsed = obj_io._parse_obj(name)
            assert len(parsed[2]) == 3 * len(pf)                                                  # vt count
            tile_w, tile_h = tref.atlas_tiles(len(pf))
            png = png_ref.read_png(os.path.join(export_dir, sub, f"k1.{what}.png")) if len(pf) < 2000 else \
                obj_io.read_png_plain(os.path.join(export_dir, sub, f"k1.{what}.png"))
            assert png.shape == (tile_h * 16, tile_w * 16, 3)
            assert float(t.min()) >= 0 and float(t.max()) <= 1 and float(t.std()) > 0


class _Body:
    """what save_outputs reads of a body model: the vertices, the faces and the three parameter tensors"""

    def __init__(self, verts, faces):
        self.verts, self.faces = verts, faces
        self.pose, self.betas, self.trans = torch.zeros(1, 72), torch.zeros(1, 10), torch.zeros(1, 3)

    def forget(self):
        pass

    def __call__(self):
        return (self.verts,)


def test_export_of_small_meshes_and_missing_inputs(tmp_path, monkeypatch):
    """save_outputs with the switch on, on a sphere for the body and a box for the object: the files hold the PLYs' vertices and
    the cubes photo_mesh_textures computes with the plain mesh colours; without the batch's images it raises"""
    from chore_amd.recon.assets import read_ply
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    from chore_amd.render import load_obj
    from chore_amd.utils import render_utils as ru
    from meshes import icosphere
    from ordinal_depth_ref import BOX_FACES, box_verts
    fitter = ReconFitterBase.from_parts(device="cuda:0", scan_verts=box_verts((0.15, 0.2, 0.15)), scan_faces=BOX_FACES)
    fitter.outpath = str(tmp_path)
    sv, sf = icosphere(1, 0.25, (0.0, -0.35, 2.2))
    body = _Body(torch.as_tensor(sv, dtype=torch.float32).cuda()[None], torch.as_tensor(np.asarray(sf)).cuda())
    rng = np.random.default_rng(4)
    img = np.ones((1, 5, 512, 512), np.float32)
    img[0, :3] = rng.uniform(0, 1, (3, 512, 512))
    images = torch.from_numpy(img).cuda()
    cc = torch.tensor([[fitter.camera.cx_px, fitter.camera.cy_px]], dtype=torch.float32)
    R, t, s = torch.eye(3).cuda()[None], torch.tensor([[0.0, 0.35, 2.2]]).cuda(), torch.ones(1).cuda()
    paths = [os.path.join("data", "seq", "t0001.000", "k1.color.jpg")]
    monkeypatch.setattr(ReconFitterBase, "EXPORT_TEXTURED_OBJ", True)
    with pytest.raises(RuntimeError, match="EXPORT_TEXTURED_OBJ needs"):
        fitter.save_outputs(body, R, t, paths, "test", 1, obj_s=s)
    with pytest.raises(RuntimeError, match="EXPORT_TEXTURED_OBJ needs"):
        fitter.save_outputs(_Body(body.verts, None), R, t, paths, "test", 1, obj_s=s, images=images, crop_centers=cc)
    fitter.save_outputs(body, R, t, paths, "test", 1, obj_s=s, images=images, crop_centers=cc)
    folder = os.path.join(str(tmp_path), "seq", "t0001.000", "test")
    meshes = [ru.Mesh(*read_ply(os.path.join(folder, "k1.%s.ply" % w))) for w in ("smpl", "object")]
    verts, faces, colour = ru.mesh_tensors(meshes, ru.SMPL_OBJ_COLOR_LIST, images.device)
    want = ru.photo_mesh_textures(images[0], cc[0], verts, faces, colour[:, :, 0, 0, 0, :], depth_bias=fitter.VIEW_POINT_BIAS,
                                  camera=fitter.camera)[0].cpu().numpy()
    assert (np.abs(want - colour[0].cpu().numpy()).max(-1) > 0.05).mean() > 0.1            # the photo is on the meshes
    first = 0
    for w, mesh in zip(("smpl", "object"), meshes):
        v, f, tex = load_obj(os.path.join(folder, "k1.%s.obj" % w), normalization=False, load_texture=True,
                             texture_wrapping="CLAMP_TO_EDGE")
        assert np.array_equal(f.cpu().numpy(), mesh.f) and np.abs(v.cpu().numpy() - mesh.v).max() <= 1e-8 + 1e-6
        cubes = want[first:first + len(mesh.f)]
        first += len(mesh.f)
        for c in ((3, 0, 0), (0, 3, 0), (0, 0, 3)):
            assert np.abs(tex.cpu().numpy()[(slice(None),) + c] - cubes[(slice(None),) + c]).max() <= 0.5 / 255 + 5e-4, (w, c)


def test_render_photo_views_unchanged():
    """render_photo_views is the composition it was before its texture computation moved into photo_mesh_textures, bit for bit"""
    from chore_amd import render as nr
    from chore_amd.model.camera import KinectColorCamera
    from chore_amd.utils import render_utils as ru
    from meshes import icosphere
    from ordinal_depth_ref import BOX_FACES, box_verts, rot_xyz
    cam = KinectColorCamera()
    rng = np.random.default_rng(3)
    img = np.ones((5, 512, 512), np.float32)
    img[:3] = rng.uniform(0, 1, (3, 512, 512))
    sv, sf = icosphere(2, 0.25, (0.0, -0.35, 2.2))
    bv = box_verts((0.15, 0.2, 0.15)).astype(np.float64) @ rot_xyz(0, np.pi / 4, 0).astype(np.float64).T + [0.0, 0.35, 2.2]
    images, cc = torch.from_numpy(img).cuda(), torch.tensor([cam.cx_px, cam.cy_px], dtype=torch.float32).cuda()
    meshes = [ru.Mesh(v=sv, f=sf), ru.Mesh(v=bv, f=BOX_FACES)]
    view = ru.render_photo_views(images, cc, meshes, ru.SMPL_OBJ_COLOR_LIST)
    # the composition, from the public pieces
    verts, faces, textures = ru.mesh_tensors(meshes, ru.SMPL_OBJ_COLOR_LIST, images.device)
    S, near, far = ru.CLOUD_VIEW_SIZE, nr.renderer.DEFAULT_NEAR, nr.renderer.DEFAULT_FAR
    front = ru._over_photo({"rgb": torch.zeros(1, 3, S, S, device="cuda"), "alpha": torch.zeros(1, S, S, device="cuda")}, images, S)
    side = ru.setup_side_renderer(2.0, 0., 90.)
    _, place = ru._side_normalisation(verts[0], 1.5)
    side_verts = place(verts[0])[None]
    light = nr.face_light(nr.vertices_to_faces(side_verts, faces), side.light_intensity_ambient, side.light_intensity_directional,
                          side.light_color_ambient, side.light_color_directional, side.light_direction)
    ndc = ru._input_view_ndc(cam, verts[0], cc)
    depth = nr.sample_depth(nr.vertices_to_faces(ndc, torch.cat((faces, faces.flip(-1)), dim=1)), S, near, far)
    photo = images[:3].detach().float().clamp(0, 1)[None]
    tex = nr.photo_textures(nr.vertices_to_faces(ndc, faces), depth, photo, textures[:, :, 0, 0, 0, :] * light, ru.TEXTURE_SIZE, 0.02,
                            near, far, align_corners=True)
    tri, tex, _, _ = side._prepare_faces(side_verts, faces, tex, (None,) * 5)
    rgb = nr.rasterize_rgbad(tri, tex, None, side.image_size, side.anti_aliasing, side.near, side.far, side.rasterizer_eps,
                             side.background_color)["rgb"]
    assert np.array_equal(view, np.concatenate([front, ru._side_crop(rgb, S)], axis=1))
    # the exported textures: the same photo texels, the plain mesh colour where the camera sees nothing
    plain = ru.photo_mesh_textures(images, cc, verts, faces, textures[:, :, 0, 0, 0, :])
    lit = ru.photo_mesh_textures(images, cc, verts, faces, textures[:, :, 0, 0, 0, :] * light)
    _, seen = nr.photo_textures(nr.vertices_to_faces(ndc, faces), depth, photo, textures[:, :, 0, 0, 0, :], ru.TEXTURE_SIZE, 0.02,
                                near, far, align_corners=True, return_visible=True)
    assert torch.equal(plain[seen], lit[seen]) and bool(seen.any()) and bool((~seen).any())
    assert torch.equal(plain[~seen], textures[~seen])
