"""Render fitted SMPL + object meshes over the input photo and from the side.

Provides the names that `utils/render_utils.py` of a CHORE checkout exports (SMPL_OBJ_COLOR_LIST, NrWrapper, cal_norm_scale,
get_faces_and_textures, get_kinect_K, setup_renderer, setup_side_renderer, align_to_input, load_mesh) with the same call
signatures and results, written against this package: the renderer is chore_amd.render.Renderer (HIP rasteriser), a mesh
is any object with `.v` (V,3) and `.f` (F,3) (`Mesh` below), PLY files are read by chore_amd.recon.assets.read_ply, and the
resize inside `align_to_input` is ImagePrep.resize (chore_prep_resize_u8; its parity with cv2.resize is unpinned, see
chore_amd/data/image_prep.py).  No cv2, psbody or neural_renderer import.  What these functions compute is pinned by
tests/golden/render_host.npz, recorded from the checkout's own module.  Not provided: setup_renderer's view='top', which
nothing in the checkout calls.

`render_fit_views` is the rendering tail of the checkout's demo.py (demo.py:37-53) in one call, from decoded arrays (file
IO stays with the caller).
"""
import os
import struct
import zlib

import numpy as np
import torch

from .. import render as nr
from ..model.camera import KinectColorCamera
from ..recon.recon_fit_base import MTURK_COLORS

SMPL_OBJ_COLOR_LIST = [
    [0.65098039, 0.74117647, 0.85882353],      # body
    [251 / 255.0, 128 / 255.0, 114 / 255.0],   # object
]
TEXTURE_SIZE = 4                               # texels per edge of a face's (uniform) colour cube
# colour camera of the Kinect at its native 2048-px width
KINECT_WIDTH = 2048
KINECT_FOCAL = (979.784, 979.840)
KINECT_CENTRE = (1018.952, 779.486)
MEAN_CROP_CENTER = (1008, 995)                 # where the in-the-wild loader moves every crop centre to
_FLIP_Y = np.array([1.0, -1.0, 1.0])           # look_at views have y up, the Kinect camera has y down
PART_COLORS = MTURK_COLORS                      # the fitter's 14 body-part colours, rows in [0,1]
CLOUD_VIEW_SIZE, CLOUD_SIDE_SIZE = 512, 640    # render_cloud_views: the input view and the side view, pixels


def write_png(path, u8):
    """an (H,W,3) RGB or (H,W) / (H,W,1) grey uint8 array as an 8-bit PNG, with zlib and struct only"""
    a = np.ascontiguousarray(u8)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.size == 0:
        raise ValueError("write_png takes a non-empty uint8 array (H,W), (H,W,1) or (H,W,3), got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    colour_type = 2 if a.ndim == 3 and a.shape[2] == 3 else 0
    rows = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, -1)], axis=1)          # filter type 0 on every row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


class Mesh:
    """vertices `.v` (V,3) float64 and faces `.f` (F,3): what this module reads of a mesh"""

    def __init__(self, v=None, f=None, filename=None):
        if filename is not None:
            self.load_from_file(filename)
        if v is not None:
            self.v = np.array(v, dtype=np.float64)
        if f is not None:
            self.f = np.array(f)

    def load_from_file(self, filename):
        from ..recon.assets import read_ply
        self.v, self.f = read_ply(filename)
        return self


def load_mesh(pcfile):
    """the mesh of a PLY file, None when the file does not exist"""
    return Mesh(filename=pcfile) if os.path.isfile(pcfile) else None


def icosphere_mesh(center, radius, subdiv=2):
    """a sphere as a `Mesh`: the icosahedron with every triangle split in four `subdiv` times and the new vertices pushed out
    to the sphere (20 * 4**subdiv faces, wound so that the normals point outwards).  The centre markers of the debug views."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    # twelve vertices on three golden rectangles; five faces round vertex 0, the five next to them, and the same below
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                  (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], dtype=np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
                  (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
                  (8, 6, 7), (9, 8, 1)], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(int(subdiv)):
        edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)       # (3F,2): ab, bc, ca of every face
        uniq, inv = np.unique(edges, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        ab, bc, ca = (len(v) + inv.reshape(-1)).reshape(3, len(f))
        v = np.concatenate([v, mid / np.linalg.norm(mid, axis=1, keepdims=True)])
        a, b, c = f.T
        f = np.concatenate([np.stack(t, 1) for t in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return Mesh(v=v * float(radius) + np.asarray(center, dtype=np.float64).reshape(1, 3), f=f)


def cal_norm_scale(meshes, maxd=2.0):
    """the factor that brings the longest edge of the meshes' common bounding box to `maxd`"""
    pts = np.concatenate([np.asarray(m.v) for m in meshes], axis=0)
    extent = pts.max(axis=0) - pts.min(axis=0)
    return (maxd / extent).min()


def get_faces_and_textures(verts_list, faces_list, colors_list=SMPL_OBJ_COLOR_LIST):
    """several meshes as one: verts_list [(B,V_i,3)], faces_list [(F_i,3) int], one colour each -> faces (1, sum B F_i, 3)
    that index the vertices concatenated mesh after mesh, and uniform textures (1, sum B F_i, 4, 4, 4, 3)"""
    faces_out, tex_out, first = [], [], 0
    for verts, faces, color in zip(verts_list, faces_list, colors_list):
        copies, per_copy = verts.shape[0], verts.shape[1]
        starts = first + per_copy * torch.arange(copies, device=verts.device)
        shifted = faces.unsqueeze(0) + starts.view(copies, 1, 1).to(faces.dtype)
        faces_out.append(shifted.reshape(-1, 3))
        first += copies * per_copy
        cube = torch.tensor(color, dtype=torch.float32, device=verts.device).expand(TEXTURE_SIZE, TEXTURE_SIZE, TEXTURE_SIZE, 3)
        tex_out.append(cube.unsqueeze(0).repeat(copies * faces.shape[0], 1, 1, 1, 1))
    return torch.cat(faces_out, 0).unsqueeze(0), torch.cat(tex_out, 0).unsqueeze(0)


def get_kinect_K(image_size=2048):
    """(K (1,3,3), ratio): the Kinect intrinsics for a rendering `image_size` pixels wide"""
    ratio = image_size / float(KINECT_WIDTH)
    K = torch.eye(3, dtype=torch.float32)
    K[0, 0], K[1, 1] = KINECT_FOCAL[0] * ratio, KINECT_FOCAL[1] * ratio
    K[0, 2], K[1, 2] = KINECT_CENTRE[0] * ratio, KINECT_CENTRE[1] * ratio
    return K.unsqueeze(0), ratio


def _soft_light(renderer, ambient, direction):
    # The checkout stores the directional intensity 0.3 under `light_intensity_direction`, a name its renderer never reads, so
    # there the constructor's 0.5 stays in force.  Here the 0.3 is applied (and kept under the other name too): with the
    # un-normalised direction of the front view the light factor spans 0.4 .. 0.4 + 0.3 * 1.5.
    renderer.light_intensity_ambient = ambient
    renderer.light_intensity_directional = renderer.light_intensity_direction = 0.3
    renderer.light_direction = direction
    renderer.background_color = [1, 1, 1]
    return renderer


def setup_renderer(view='front', rotate=False, image_size=2048):
    """the Kinect colour camera as a square `image_size` rendering (the 2048 x 1536 frame is its upper part);
    rotate=True turns the camera by 180 degrees about its axis"""
    if view != 'front':
        raise NotImplementedError("only the front view is provided, got view=%r" % (view,))
    K, ratio = get_kinect_K(image_size)
    turn = -1.0 if rotate else 1.0
    R = torch.diag(torch.tensor([turn, turn, 1.0])).unsqueeze(0)
    renderer = nr.Renderer(image_size=image_size, K=K, R=R, t=torch.zeros(1, 3), orig_size=KINECT_WIDTH * ratio)
    return _soft_light(renderer, 0.4, [1, 0.5, 1])


def setup_side_renderer(dist=2.0, elev=45., azim=90., image_size=640):
    """a look_at camera on a sphere around the origin, lit from where it stands; for meshes centred at the origin"""
    renderer = nr.Renderer(camera_mode='look_at', image_size=image_size)
    renderer.eye = nr.get_points_from_angles(dist, elev, azim)
    return _soft_light(renderer, 0.5, [c / 2.2 for c in renderer.eye])


class NrWrapper:
    """front renderer plus the tensor preparation of a list of meshes"""

    def __init__(self, device='cuda:0', image_size=1024, colors=None):
        self.device = device
        self.colors = [list(c) for c in SMPL_OBJ_COLOR_LIST] if colors is None else colors
        self.smpl_color, self.obj_color = SMPL_OBJ_COLOR_LIST
        self.front_renderer = setup_renderer(image_size=image_size)

    def render(self, renderer, verts, faces, texts):
        """-> image (S,S,3) float in [0,1], mask (S,S) bool: the pixels with any covered sample"""
        rgb, _, alpha = renderer.render(vertices=verts, faces=faces, textures=texts)
        image = rgb[0].permute(1, 2, 0).clamp(0, 1).cpu().numpy()
        return image, (alpha[0] != 0).cpu().numpy()

    def render_meshes(self, renderer, meshes: list, colors=None):
        """render the meshes (body, object, ...) in self.colors or `colors`"""
        return self.render(renderer, *self.prepare_render(meshes, colors))

    def prepare_render(self, meshes, colors=None):
        """-> vertices (1, sum V, 3) float32, faces (1, sum F, 3) int32, textures (1, sum F, 4, 4, 4, 3) on self.device"""
        return mesh_tensors(meshes, self.colors if colors is None else colors, self.device)

    def render_points(self, renderer, clouds, colors, world_radius):
        """several point clouds in ONE splat call, so that occlusion between them is resolved per sample and nothing has to
        be composited: clouds [(N_i,3) world points], colors [one (3,) colour or (N_i,3) per cloud], world_radius metres, one
        number for all or one per cloud.  -> image (S,S,3) float in [0,1], coverage (S,S) float in [0,1]"""
        pts, col, rad = concat_clouds(clouds, colors, world_radius, self.device)
        rgb, _, alpha = renderer.render_points(pts[None], col[None], world_radius=rad[None])
        return rgb[0].permute(1, 2, 0).clamp(0, 1).cpu().numpy(), alpha[0].cpu().numpy()

    def render_scene(self, renderer, meshes, clouds, colors, world_radius, mesh_colors=None, mesh_opacity=1.0,
                     point_depth_bias=0.0, face_layers=1):
        """meshes and point clouds in ONE scene call, occluding each other per sample: meshes / mesh_colors as `render_meshes`
        takes them, mesh_opacity one number for all or one per mesh, clouds / colors / world_radius as `render_points` does,
        point_depth_bias in metres (Renderer.render_scene); face_layers > 1: a translucent mesh shows up to that many meshes, the
        nearest face of each (`mesh_face_group`).  -> image (S,S,3) float in [0,1], coverage (S,S) float in [0,1]"""
        verts, faces, textures = self.prepare_render(meshes, mesh_colors)
        pts, col, rad = concat_clouds(clouds, colors, world_radius, self.device)
        used = self.colors if mesh_colors is None else mesh_colors
        rgb, _, alpha = renderer.render_scene(verts, faces, textures, pts[None], col[None], world_radius=rad[None],
                                              face_opacity=mesh_face_opacity(meshes, mesh_opacity, self.device, used),
                                              point_depth_bias=point_depth_bias, face_layers=face_layers,
                                              face_group=mesh_face_group(meshes, self.device, used) if face_layers > 1 else None)
        return rgb[0].permute(1, 2, 0).clamp(0, 1).cpu().numpy(), alpha[0].cpu().numpy()

    def render_masks(self, renderer, meshes):
        """the mask of every mesh as seen and alone, in ONE instances call (Renderer.render_instances; the mesh index is the
        face group, `mesh_face_group`): meshes with .v / .f, at most 8
        -> visible (M,S,S) float coverage of mesh i where no other mesh is in front, full (M,S,S) its coverage with the other
        meshes taken away, group_samples (M,2) int32 samples of each; device tensors"""
        verts, faces = mesh_geometry(meshes, self.device)
        out = renderer.render_instances(verts, faces, mesh_face_group(meshes, self.device), len(meshes))
        return out["visible"][0], out["full"][0], out["group_samples"][0]

    def prepare_side_rend(self, meshes, maxd=1.5, colors=None):
        """tensors for setup_side_renderer: y flipped, scaled so that the bounding box measures `maxd`, centred at the
        vertex mean.  The caller's meshes are not modified.  -> faces, textures, vertices"""
        scaled = self.normalize_meshes(self.rotate_meshes(meshes), maxd=maxd)
        verts, faces, textures = self.prepare_render(scaled, colors=colors)
        return faces, textures, verts - verts.mean(dim=1)

    @staticmethod
    def normalize_meshes(meshes, maxd=2.0, ret_scale=False):
        """scale the meshes IN PLACE by cal_norm_scale(meshes, maxd); returns them (and the scale on request)"""
        scale = cal_norm_scale(meshes, maxd)
        for mesh in meshes:
            mesh.v = scale * np.asarray(mesh.v)
        return (meshes, scale) if ret_scale else meshes

    def rotate_meshes(self, meshes):
        """copies of the meshes with y flipped"""
        flipped = [self.copy_mesh(m) for m in meshes]
        for mesh in flipped:
            mesh.v = mesh.v * _FLIP_Y
        return flipped

    def copy_mesh(self, mesh):
        """an independent Mesh with the vertices, faces and vertex colours (`vc`) of `mesh`, as far as it has them"""
        twin = Mesh(v=mesh.v, f=getattr(mesh, 'f', None))
        if hasattr(mesh, 'vc'):
            twin.vc = np.array(mesh.vc)
        return twin


def mesh_tensors(meshes, colors, device):
    """meshes with .v / .f and one colour each -> vertices (1, sum V, 3) float32, faces (1, sum F, 3) int32, uniform textures
    (1, sum F, 4, 4, 4, 3) on `device`; a mesh without a colour is left out (zip)"""
    pairs = list(zip(meshes, colors))
    verts = [torch.as_tensor(np.asarray(m.v), dtype=torch.float32).to(device)[None] for m, _ in pairs]
    faces = [torch.as_tensor(np.asarray(m.f).astype(np.int32)).to(device) for m, _ in pairs]
    all_faces, textures = get_faces_and_textures(verts, faces, colors_list=[c for _, c in pairs])
    return torch.cat(verts, dim=1), all_faces, textures


def mesh_geometry(meshes, device):
    """meshes with .v / .f -> vertices (1, sum V, 3) float32 and faces (1, sum F, 3) int32 that index them, mesh after mesh,
    on `device`: `mesh_tensors` without the textures"""
    verts = [torch.as_tensor(np.asarray(m.v), dtype=torch.float32).to(device) for m in meshes]
    first = np.cumsum([0] + [len(v) for v in verts[:-1]])
    faces = [torch.as_tensor(np.asarray(m.f).astype(np.int32)).to(device) + int(o) for m, o in zip(meshes, first)]
    return torch.cat(verts)[None], torch.cat(faces)[None]


def mesh_face_opacity(meshes, mesh_opacity, device, colors=None):
    """one number for all meshes or one per mesh -> (1, sum F) float32, in the face order of `mesh_tensors`.  With `colors`
    (what `mesh_tensors` gets) a mesh without a colour is an error here, since `mesh_tensors` would leave it out"""
    if not isinstance(mesh_opacity, (list, tuple)):
        mesh_opacity = [mesh_opacity] * len(meshes)
    if len(mesh_opacity) != len(meshes) or (colors is not None and len(colors) < len(meshes)):
        raise ValueError("%d meshes need %d opacities (got %d) and as many colours (got %s)"
                         % (len(meshes), len(meshes), len(mesh_opacity), "none" if colors is None else len(colors)))
    return torch.cat([torch.full((len(m.f),), float(o), device=device) for m, o in zip(meshes, mesh_opacity)])[None]


def mesh_face_group(meshes, device, colors=None):
    """the mesh index of every face -> (1, sum F) int32, in the face order of `mesh_tensors`: the `face_group` under which a
    translucent mesh counts as ONE layer of the scene rasteriser.  `colors` as in `mesh_face_opacity`"""
    if colors is not None and len(colors) < len(meshes):
        raise ValueError("%d meshes need as many colours (got %d)" % (len(meshes), len(colors)))
    return torch.cat([torch.full((len(m.f),), i, dtype=torch.int32, device=device) for i, m in enumerate(meshes)])[None]


def concat_clouds(clouds, colors, radii, device):
    """clouds [(N_i,3)], colors [(3,) or (N_i,3)], radii a number or one per cloud -> points (N,3), colours (N,3), radii (N,)
    float32 tensors on `device`, cloud after cloud (tensors already there are not copied through the host)"""
    if not isinstance(radii, (list, tuple)):
        radii = [radii] * len(clouds)
    on = lambda x: torch.as_tensor(x, dtype=torch.float32, device=device) if not torch.is_tensor(x) else \
        x.detach().to(device=device, dtype=torch.float32)                  # noqa: E731
    pts, col, rad = [], [], []
    for p, c, r in zip(clouds, colors, radii):
        p, c = on(p).reshape(-1, 3), on(c)
        pts.append(p)
        col.append(c.reshape(1, 3).expand(len(p), 3) if c.numel() == 3 else c.reshape(len(p), 3))
        rad.append(torch.full((len(p),), float(r), device=device))
    return torch.cat(pts), torch.cat(col), torch.cat(rad)


def _input_view_ndc(camera, pts, crop_center_b):
    """camera-space points (N,3) through the network's camera -> (1,N,3) [u, v, z]: `camera.project_points` gives
    [nx, ny, z] and the rasterisers take v = -ny, since their output rows are flipped"""
    proj = camera.project_points(pts[None], crop_center_b.to(pts.device).float().reshape(1, 2)).transpose(1, 2)     # (1,N,3)
    return torch.stack([proj[..., 0], -proj[..., 1], proj[..., 2]], dim=-1)


def _append_markers(ndc, col, rad_px, markers2d, S, near):
    """the 2-D markers as splats at a depth just inside `near`, so they win every sample they cover"""
    dev = ndc.device
    for xy, c, r in markers2d or ():
        xy = torch.as_tensor(np.asarray(xy.detach().cpu()) if torch.is_tensor(xy) else np.asarray(xy), dtype=torch.float32)
        xy = xy.reshape(-1, 2).to(dev)
        u, v = (2 * xy[:, 0] + 1) / S - 1, -((2 * xy[:, 1] + 1) / S - 1)
        ndc = torch.cat([ndc, torch.stack([u, v, torch.full_like(u, near * 1.01)], -1)[None]], 1)
        col = torch.cat([col, torch.tensor(c, dtype=torch.float32, device=dev).reshape(1, 3).expand(len(xy), 3)])
        rad_px = torch.cat([rad_px, torch.full((1, len(xy)), float(r), device=dev)], 1)
    return ndc, col, rad_px


def _over_photo(out, images_b, S):
    """a rasteriser's rgb / alpha over the frame's photo -> (S,S,3) uint8.  The colours are weighted by their coverage already"""
    dev = images_b.device
    photo = images_b[:3].detach().float().clamp(0, 1)
    if photo.shape[1] != S or photo.shape[2] != S:         # nearest-neighbour to the view's size
        iy = (torch.arange(S, device=dev) * photo.shape[1]) // S
        ix = (torch.arange(S, device=dev) * photo.shape[2]) // S
        photo = photo[:, iy][:, :, ix]
    front = out["rgb"][0] + (1 - out["alpha"][0])[None] * photo
    return (front.permute(1, 2, 0).clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()


def _side_normalisation(pts, maxd):
    """prepare_side_rend on the device: y flipped, the bounding box of the finite points scaled to `maxd` (cal_norm_scale),
    centred at their mean -> (scale, place) with place(x) = scale * (x * _FLIP_Y - mean)"""
    flip = torch.tensor(_FLIP_Y, dtype=torch.float32, device=pts.device)
    flipped = pts * flip
    keep = torch.isfinite(flipped).all(dim=1, keepdim=True)
    big = torch.finfo(torch.float32).max
    extent = torch.where(keep, flipped, -big).amax(0) - torch.where(keep, flipped, big).amin(0)
    scale = (maxd / extent.clamp(min=1e-12)).min()
    mean = torch.where(keep, flipped, 0.0).sum(0) / keep.sum().clamp(min=1)
    return scale, lambda x: scale * (x * flip - mean)


def _side_crop(rgb, S):
    """the middle S rows of a rendering (1,3,H,W) -> (S,W,3) uint8"""
    side = (rgb[0].permute(1, 2, 0).clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
    top = (side.shape[0] - S) // 2
    return side[top:top + S]


def render_cloud_views(images_b, crop_center_b, clouds, colors, radii, markers2d=None, side_renderer=None, camera=None,
                       maxd=1.5, min_radius_px=1.0):
    """the fitter's point clouds of ONE frame in two views -> (512, 512 + 640, 3) uint8.

    images_b (C,H,W) network input of the frame (channels 0..2 RGB in [0,1]), crop_center_b (2,), clouds / colors / radii as
    `concat_clouds` takes them (camera-space points, world radii in metres), markers2d [(xy (M,2) pixel positions in the 512-px
    network input, colour (3,), radius in pixels)].
    Input view (left, 512 px): the clouds through the network's own camera -- `camera.project_points` gives [nx, ny, z] and
    the splats take v = -ny, since the rasterisers' output rows are flipped -- alpha-blended over the input photo; the
    markers are splats at a depth just inside `near`, so they win every sample they cover.
    Side view (right, the middle 512 rows of a 640-px rendering): the same clouds through setup_side_renderer(2.0, 0., 90.) after
    the y-flip, scaling (bounding box -> `maxd`) and centring of NrWrapper.prepare_side_rend.
    No disc is drawn smaller than `min_radius_px`: a scattered cloud scales the side view down, and points must not vanish."""
    dev = images_b.device
    camera = KinectColorCamera() if camera is None else camera
    pts, col, rad = concat_clouds(clouds, colors, radii, dev)
    S, near = CLOUD_VIEW_SIZE, nr.renderer.DEFAULT_NEAR
    ndc = _input_view_ndc(camera, pts, crop_center_b)
    focal = camera.fx_px * S / camera.crop_size
    rad_px = nr.world_radius_to_pixels(rad[None], ndc[..., 2], focal).clamp(min=min_radius_px)
    n = len(pts)
    ndc, col, rad_px = _append_markers(ndc, col, rad_px, markers2d, S, near)
    out = nr.splat_points(ndc, col[None], rad_px, S, True, near, nr.renderer.DEFAULT_FAR, ambient=0.6)
    front = _over_photo(out, images_b, S)

    side_renderer = setup_side_renderer(2.0, 0., 90.) if side_renderer is None else side_renderer
    scale, place = _side_normalisation(pts, maxd)
    side_ndc = side_renderer.transform(place(pts)[None])
    side_px = nr.world_radius_to_pixels((rad * scale)[None], side_ndc[..., 2], side_renderer.focal_pixels())
    rgb = nr.splat_points(side_ndc, col[None, :n], side_px.clamp(min=min_radius_px), side_renderer.image_size,
                          side_renderer.anti_aliasing, side_renderer.near, side_renderer.far,
                          background_color=side_renderer.background_color)["rgb"]
    return np.concatenate([front, _side_crop(rgb, S)], axis=1)


def render_scene_views(images_b, crop_center_b, meshes, mesh_colors, mesh_opacity, clouds, colors, radii, markers2d=None,
                       point_depth_bias=0.0, side_renderer=None, camera=None, maxd=1.5, min_radius_px=1.0, face_layers=1):
    """meshes AND point clouds of ONE frame in the two views of `render_cloud_views` -> (512, 512 + 640, 3) uint8, each view one
    scene call (chore_scene_fwd), so meshes and points occlude each other per sample.

    meshes with .v (camera space) / .f, mesh_colors one colour each, mesh_opacity one number for all or one per mesh.  With
    face_layers = 1 a translucent face shows the nearest point behind it or the background, never another face; with
    face_layers > 1 (chore_scene_layers_fwd) a translucent mesh shows up to that many meshes, each as one layer: the mesh index
    is the face group.  point_depth_bias in metres (scaled with the side view); the rest as `render_cloud_views` takes it.  The meshes go through exactly the clouds'
    transforms: the network's camera with v = -ny in the input view (lit like setup_renderer's front view), and in the side
    view the y-flip, scale and centring, which are computed from the cloud points and the mesh vertices together."""
    if not meshes:
        raise ValueError("render_scene_views needs at least one mesh; render_cloud_views draws clouds alone")
    dev = images_b.device
    camera = KinectColorCamera() if camera is None else camera
    pts, col, rad = concat_clouds(clouds, colors, radii, dev)
    verts, faces, textures = mesh_tensors(meshes, mesh_colors, dev)
    opacity = mesh_face_opacity(meshes, mesh_opacity, dev, mesh_colors)
    group = mesh_face_group(meshes, dev, mesh_colors) if face_layers > 1 else None
    # both windings of a face get its group where a renderer fills the back, as they get its opacity
    wound = lambda r: torch.cat((group, group), dim=1) if group is not None and r.fill_back else group      # noqa: E731
    S, near, far = CLOUD_VIEW_SIZE, nr.renderer.DEFAULT_NEAR, nr.renderer.DEFAULT_FAR
    ndc = _input_view_ndc(camera, pts, crop_center_b)
    focal = camera.fx_px * S / camera.crop_size
    rad_px = nr.world_radius_to_pixels(rad[None], ndc[..., 2], focal).clamp(min=min_radius_px)
    n = len(pts)
    ndc, col, rad_px = _append_markers(ndc, col, rad_px, markers2d, S, near)
    front_light = _soft_light(nr.Renderer(camera_mode='look_at', image_size=S), 0.4, [1, 0.5, 1])      # carries the light only
    tri, tex, light, op = front_light._prepare_faces(verts, faces, textures, (), opacity,
                                                     projected=_input_view_ndc(camera, verts[0], crop_center_b))
    out = nr.rasterize_scene(tri, tex, light, ndc, col[None], rad_px, op, point_depth_bias, S, True, near, far, ambient=0.6,
                             face_layers=face_layers, face_group=wound(front_light))
    front = _over_photo(out, images_b, S)

    side_renderer = setup_side_renderer(2.0, 0., 90.) if side_renderer is None else side_renderer
    scale, place = _side_normalisation(torch.cat([pts, verts[0]]), maxd)
    side_ndc = side_renderer.transform(place(pts)[None])
    side_px = nr.world_radius_to_pixels((rad * scale)[None], side_ndc[..., 2], side_renderer.focal_pixels())
    tri, tex, light, op = side_renderer._prepare_faces(place(verts[0])[None], faces, textures, (None,) * 5, opacity)
    rgb = nr.rasterize_scene(tri, tex, light, side_ndc, col[None, :n], side_px.clamp(min=min_radius_px), op,
                             float(point_depth_bias * scale), side_renderer.image_size, side_renderer.anti_aliasing,
                             side_renderer.near, side_renderer.far, side_renderer.rasterizer_eps,
                             background_color=side_renderer.background_color, face_layers=face_layers,
                             face_group=wound(side_renderer))["rgb"]
    return np.concatenate([front, _side_crop(rgb, S)], axis=1)


def photo_mesh_textures(images_b, crop_center_b, verts, faces, fallback, texture_size=TEXTURE_SIZE, depth_bias=0.02, camera=None):
    """the texture cubes (1,F,ts,ts,ts,3) of camera-space meshes coloured from the photo they were fitted to: what
    `render_photo_views` draws and what the fitter's textured OBJ export writes.  images_b (C,H,W) network input of the frame
    (channels 0..2 RGB in [0,1]), crop_center_b (2,), verts (1,V,3) / faces (1,F,3) as `mesh_tensors` gives them, fallback
    (1,F,3): the colour of a texel the network's camera does not see.  Every other texel takes the photo's colour
    (`nr.photo_textures` on the `_input_view_ndc` triangles, align_corners=True like the network's own grid_sample, visibility
    on the CLOUD_VIEW_SIZE grid over both windings)."""
    camera = KinectColorCamera() if camera is None else camera
    S, near, far = CLOUD_VIEW_SIZE, nr.renderer.DEFAULT_NEAR, nr.renderer.DEFAULT_FAR
    ndc = _input_view_ndc(camera, verts[0], crop_center_b)
    depth = nr.sample_depth(nr.vertices_to_faces(ndc, torch.cat((faces, faces.flip(-1)), dim=1)), S, near, far)
    photo = images_b[:3].detach().float().clamp(0, 1)[None]
    return nr.photo_textures(nr.vertices_to_faces(ndc, faces), depth, photo, fallback, texture_size, depth_bias, near, far,
                             align_corners=True)


def render_photo_views(images_b, crop_center_b, meshes, mesh_colors, texture_size=TEXTURE_SIZE, depth_bias=0.02, side_renderer=None,
                       camera=None, maxd=1.5):
    """the fitted meshes of ONE frame wearing the photo they were fitted to -> (512, 512 + 640, 3) uint8: the input photo on the
    left, the side view of `render_scene_views` (same y-flip, scale and centring) on the right, where a misfit shows as the wrong
    patch of image on the wrong part of a mesh.

    images_b (C,H,W) network input of the frame (channels 0..2 RGB in [0,1]), crop_center_b (2,), meshes with .v (camera space)
    / .f, mesh_colors one colour each.  Every texel the network's camera sees takes the photo's colour there
    (`nr.photo_textures` on the `_input_view_ndc` triangles, align_corners=True like the network's own
    grid_sample, visibility on the CLOUD_VIEW_SIZE grid over both windings); every other texel -- hidden, out of the crop -- takes
    the mesh colour times the side renderer's face light.  The side view is then rasterised WITHOUT light, so the photo is not
    lit a second time.  depth_bias: metres; 0.02 is the fitter's VIEW_POINT_BIAS, not tuned."""
    if not meshes:
        raise ValueError("render_photo_views needs at least one mesh")
    dev = images_b.device
    camera = KinectColorCamera() if camera is None else camera
    verts, faces, textures = mesh_tensors(meshes, mesh_colors, dev)
    S = CLOUD_VIEW_SIZE
    blank = {"rgb": torch.zeros(1, 3, S, S, device=dev), "alpha": torch.zeros(1, S, S, device=dev)}
    front = _over_photo(blank, images_b, S)

    side_renderer = setup_side_renderer(2.0, 0., 90.) if side_renderer is None else side_renderer
    _, place = _side_normalisation(verts[0], maxd)
    side_verts = place(verts[0])[None]
    light = nr.face_light(nr.vertices_to_faces(side_verts, faces), side_renderer.light_intensity_ambient,
                          side_renderer.light_intensity_directional, side_renderer.light_color_ambient,
                          side_renderer.light_color_directional, side_renderer.light_direction)
    textures = photo_mesh_textures(images_b, crop_center_b, verts, faces, textures[:, :, 0, 0, 0, :] * light, texture_size,
                                   depth_bias, camera)
    tri, tex, _, _ = side_renderer._prepare_faces(side_verts, faces, textures, (None,) * 5)
    rgb = nr.rasterize_rgbad(tri, tex, None, side_renderer.image_size, side_renderer.anti_aliasing, side_renderer.near,
                             side_renderer.far, side_renderer.rasterizer_eps, side_renderer.background_color)["rgb"]
    return np.concatenate([front, _side_crop(rgb, S)], axis=1)


def _resize_u8(img, dsize, device):
    """cv2.resize(img, dsize) for uint8 images; equal sizes are a copy (as in cv2)"""
    if (img.shape[1], img.shape[0]) == (int(dsize[0]), int(dsize[1])):
        return img.copy()
    from ..data.image_prep import ImagePrep
    return ImagePrep(device=device).resize(np.ascontiguousarray(img), dsize).cpu().numpy()


def _window(img, lo, hi, frame, fill):
    """the window [lo, hi) (x, y corners) of the part of `img` inside `frame` (width, height); outside is `fill`"""
    (x0, y0), (x1, y1) = (int(c) for c in lo), (int(c) for c in hi)
    cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, frame[0]), min(y1, frame[1])
    out = np.full((y1 - y0, x1 - x0) + img.shape[2:], fill, dtype=img.dtype)
    if cx1 > cx0 and cy1 > cy0:
        out[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0] = img[cy0:cy1, cx0:cx1]
    return out


def align_to_input(crop_info, height, rend, train_crop_size, width, mean_cent=False, pad_value=255, device="cuda:0"):
    """Bring a rendering of the square camera frame into the frame of the (resized) input photo.

    The network saw a crop of `train_crop_size` pixels of the photo, which the loader had cut with side crop_info['crop_size']
    around crop_info['crop_center'] and -- for in-the-wild data, mean_cent=True -- moved to MEAN_CROP_CENTER.  So the same
    window is cut out of `rend` ((S,S) or (S,S,3) uint8, of which the `width` x `height` part counts), resized to the
    loader's crop size and pasted at the crop centre into a canvas of crop_info['rgb_newsize'] = (w, h) filled with `pad_value`.
    -> (h,w) or (h,w,3) uint8"""
    w, h = (int(s) for s in crop_info['rgb_newsize'])
    centre = np.asarray(crop_info['crop_center']).astype(int)
    side = int(crop_info['crop_size'][0])
    half = train_crop_size // 2
    seen_at = np.array(MEAN_CROP_CENTER) if mean_cent else centre
    patch = _window(rend, seen_at - half, seen_at + half, (width, height), pad_value)
    patch = _resize_u8(patch, (side, side), device)
    # paste the patch with its corner at centre - side // 2, clipped to the canvas
    x0, y0 = (int(c) for c in centre - side // 2)
    canvas = np.full((h, w) + rend.shape[2:], pad_value, dtype=np.uint8)
    cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x0 + side, w), min(y0 + side, h)
    if cx1 > cx0 and cy1 > cy0:
        canvas[cy0:cy1, cx0:cx1] = patch[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    return canvas


def render_fit_views(rgb_u8, crop_info, smpl_mesh, obj_mesh, load_size, nrwrapper=None, side_renderer=None, height=1536,
                     width=2048, mean_cent=True, maxd=1.8, device="cuda:0"):
    """the rendering half of the checkout's demo.py (:37-53) from decoded arrays.
    rgb_u8 (oh,ow,3) uint8 RGB photo, crop_info the loader's dict, meshes with .v / .f, load_size = args.loadSize.
    -> (overlap_u8 (oh,ow,3): the photo with the front rendering pasted where it covers, side_u8 (S,S,3): the side view
    of `side_renderer`, 640 px by default).  `nrwrapper` / `side_renderer` can be passed to reuse them across frames."""
    nrwrapper = NrWrapper(device=device, image_size=width) if nrwrapper is None else nrwrapper
    side_renderer = setup_side_renderer(2.0, 0., 90.) if side_renderer is None else side_renderer
    rgb_u8 = np.ascontiguousarray(rgb_u8)
    oh, ow = rgb_u8.shape[:2]
    photo = _resize_u8(rgb_u8, crop_info['rgb_newsize'], device)
    rend, mask = nrwrapper.render_meshes(nrwrapper.front_renderer, [smpl_mesh, obj_mesh])
    rend = (rend * 255).astype(np.uint8)
    mask = (mask * 255).astype(np.uint8)
    rend_in_photo = align_to_input(crop_info, height, rend, load_size, width, mean_cent, device=device)
    covered = align_to_input(crop_info, height, mask, load_size, width, mean_cent, 0, device=device) > 127
    photo[covered] = rend_in_photo[covered]
    overlap = _resize_u8(photo, (ow, oh), device)
    faces, texts, verts = nrwrapper.prepare_side_rend([smpl_mesh, obj_mesh], maxd=maxd)
    side, _ = nrwrapper.render(side_renderer, verts, faces, texts)
    return overlap, (side * 255).astype(np.uint8)
