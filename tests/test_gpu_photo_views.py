"""GPU: the photo-textured view of a fit (chore_amd.utils.render_utils.render_photo_views, ReconFitterBase.visualize_photo_fit) on
a synthetic frame: a photo that is green above and blue below, a sphere in its upper and a box in its lower half, both near
z = 2.2 in camera space.  No fit is run here."""
import numpy as np
import pytest
import torch

from meshes import icosphere
from ordinal_depth_ref import BOX_FACES, box_verts, rot_xyz

pytestmark = pytest.mark.gpu

GREEN, BLUE = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)


def _near(img, colour, tol=3):
    """how many pixels of the uint8 image lie within `tol` levels of `colour` (0..1)"""
    return int((np.abs(img.astype(np.int32) - np.round(np.asarray(colour) * 255).astype(np.int32)).max(-1) <= tol).sum())


def _shaded(img, colour, lo=0.45, hi=0.85, tol=0.03):
    """how many pixels are `colour` times a light factor in [lo, hi]: the side renderer's is 0.5 + 0.3 * relu(cos) * 0.91"""
    p = img.reshape(-1, 3).astype(np.float64) / 255
    c = np.asarray(colour, np.float64)
    s = (p @ c) / (c @ c)
    return int(((s > lo) & (s < hi) & (np.abs(p - s[:, None] * c).max(axis=1) < tol)).sum())


@pytest.fixture(scope="module")
def frame():
    """images (5,512,512), the crop centre at the principal point, and the two meshes: the sphere projects into rows 141..236, the
    box (turned 45 degrees about y, so the side view sees one face that looks at the camera and one that looks away) below row 256"""
    from chore_amd.model.camera import KinectColorCamera
    from chore_amd.utils.render_utils import Mesh
    cam = KinectColorCamera()
    img = np.zeros((5, 512, 512), np.float32)
    img[:3, :256] = np.float32(GREEN)[:, None, None]
    img[:3, 256:] = np.float32(BLUE)[:, None, None]
    img[3:] = 1
    sv, sf = icosphere(2, 0.25, (0.0, -0.35, 2.2))
    bv = box_verts((0.15, 0.2, 0.15)).astype(np.float64) @ rot_xyz(0, np.pi / 4, 0).astype(np.float64).T + [0.0, 0.35, 2.2]
    cc = torch.tensor([cam.cx_px, cam.cy_px], dtype=torch.float32)
    return torch.from_numpy(img).cuda(), cc.cuda(), [Mesh(v=sv, f=sf), Mesh(v=bv, f=BOX_FACES)]


def test_render_photo_views(frame):
    from chore_amd.utils.render_utils import SMPL_OBJ_COLOR_LIST, Mesh, render_photo_views
    images, cc, meshes = frame
    view = render_photo_views(images, cc, meshes, SMPL_OBJ_COLOR_LIST)
    assert view.shape == (512, 512 + 640, 3) and view.dtype == np.uint8
    photo = (images[:3].permute(1, 2, 0).clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
    assert np.array_equal(view[:, :512], photo)
    side = view[:, 512:]
    counts = {"green": _near(side, GREEN), "blue": _near(side, BLUE), "body": _shaded(side, SMPL_OBJ_COLOR_LIST[0]),
              "object": _shaded(side, SMPL_OBJ_COLOR_LIST[1]), "white": _near(side, (1, 1, 1))}
    print("side view pixels:", counts)
    # the surfaces that face the camera wear the photo, the far sides keep the mesh colours under the side renderer's light
    assert counts["green"] > 500 and counts["blue"] > 500 and counts["body"] > 500 and counts["object"] > 500
    assert counts["white"] > side.shape[0] * side.shape[1] // 2
    # the sphere is above the box in the side view too (y is flipped, then the rows are): green over blue
    rows = lambda c: np.nonzero((np.abs(side.astype(np.int32) - np.asarray(c) * 255).max(-1) <= 3).any(1))[0]     # noqa: E731
    assert rows(GREEN).max() < rows(BLUE).min()
    # moved out of the crop, nothing is seen by the camera: mesh colours only
    away = [Mesh(v=m.v + [5.0, 0.0, 0.0], f=m.f) for m in meshes]
    side = render_photo_views(images, cc, away, SMPL_OBJ_COLOR_LIST)[:, 512:]
    assert _near(side, GREEN) == 0 and _near(side, BLUE) == 0
    assert _shaded(side, SMPL_OBJ_COLOR_LIST[0]) > 1000 and _shaded(side, SMPL_OBJ_COLOR_LIST[1]) > 1000
    # a coarser cube and a bias that hides everything are taken
    assert render_photo_views(images, cc, meshes, SMPL_OBJ_COLOR_LIST, texture_size=2).shape == view.shape
    hidden = render_photo_views(images, cc, meshes, SMPL_OBJ_COLOR_LIST, depth_bias=-1e9)[:, 512:]
    assert _near(hidden, GREEN) == 0 and _near(hidden, BLUE) == 0
    with pytest.raises(ValueError):
        render_photo_views(images, cc, [], [])


def test_visualize_photo_fit(frame):
    """called directly on a fitter made from parts: the template under the fitted pose and the body's vertices with its faces"""
    from chore_amd.recon.recon_fit_base import ReconFitterBase
    from chore_amd.utils.render_utils import SMPL_OBJ_COLOR_LIST, render_photo_views
    images, cc, meshes = frame
    assert ReconFitterBase.VIEW_PHOTO_TEXTURES is False
    fitter = ReconFitterBase.from_parts(device="cuda:0", scan_verts=box_verts((0.15, 0.2, 0.15)), scan_faces=BOX_FACES)
    dd = {"images": images[None], "query_dict": {"crop_center": cc[None]}}
    body = torch.as_tensor(meshes[0].v, dtype=torch.float32).cuda()[None]
    obj = torch.as_tensor(meshes[1].v, dtype=torch.float32).cuda()[None]
    view = fitter.visualize_photo_fit(dd, obj, body, torch.as_tensor(meshes[0].f).cuda())
    assert view.shape == (512, 512 + 640, 3) and view.dtype == np.uint8
    want = render_photo_views(images, cc, meshes, SMPL_OBJ_COLOR_LIST, depth_bias=fitter.VIEW_POINT_BIAS, camera=fitter.camera)
    assert np.array_equal(view, want)
    only_object = fitter.visualize_photo_fit(dd, obj, body)                  # without faces the body is left out
    assert only_object.shape == view.shape and _near(only_object[:, 512:], GREEN) == 0 and _near(only_object[:, 512:], BLUE) > 500
