"""Textured Wavefront OBJ files in and out: neural_renderer's load_obj / load_mtl / load_textures / create_texture_image /
save_obj with their names and signatures, tensors on the device.  The two kernels are chore_load_textures and
chore_texture_atlas (csrc/texture_io.hip); their rules are written out in include/chore_hip.h.  Parsing, triangulation and the
file formats are host code, as in the reference.

Differences from the reference, all where the reference is undefined or broken:
  * every material's faces are textured in ONE launch, the UVs are wrapped in registers and never written back, and no load
    can leave an image;
  * a face corner without a `vt` index, or a file without `vt` lines, leaves that face at its material's colour (the reference
    ends up at the file's last `vt` through index -1, or raises);
  * relative (negative) OBJ indices raise ValueError (the reference indexes from the end by accident of numpy);
  * the atlas' tile rows are integers (the reference's `row = face_nums / tile_width` is a true division under today's
    torch), and tiles without a face are zero (the reference reads past `textures` there).

A file written by `save_obj` loads back only with texture_wrapping='CLAMP_TO_EDGE': the reference's REPEAT, which is the
default and is kept, sends u = 0 to 1, and the first tile column starts at u = 0.

Images are read with PIL when it imports (lazily; the package itself does not need it); without PIL a reader for
non-interlaced 8-bit grey / grey+alpha / RGB / RGBA PNG files in this module is used, and any other format raises ImportError.
"""
import ctypes
import os
import struct
import zlib

import numpy as np
import torch

from .. import _lib

texture_wrapping_dict = {'REPEAT': 0, 'MIRRORED_REPEAT': 1, 'CLAMP_TO_EDGE': 2, 'CLAMP_TO_BORDER': 3}
UNKNOWN_MATERIAL_COLOR = 0.5         # load_obj.py:77
MAX_IMAGES = 128                     # chore_load_textures' image table
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---- images -----------------------------------------------------------------------------------------------------

def _unfilter_row(kind, line, up, bpp):
    """one PNG row (int64 arrays of w * bpp bytes) -> the unfiltered row"""
    if kind == 0:
        return line
    if kind == 2:
        return (line + up) & 255
    if kind == 1:                                            # sub: a running sum per channel
        return np.cumsum(line.reshape(-1, bpp), axis=0).reshape(-1) & 255
    if kind not in (3, 4):
        raise ValueError("PNG row filter %d" % kind)
    out, src, above = [0] * len(line), line.tolist(), up.tolist()
    for x in range(len(src)):
        a = out[x - bpp] if x >= bpp else 0
        b = above[x]
        if kind == 3:
            pred = (a + b) // 2
        else:
            c = above[x - bpp] if x >= bpp else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
        out[x] = (src[x] + pred) & 255
    return np.asarray(out, np.int64)


def read_png_plain(path):
    """a non-interlaced 8-bit grey, grey+alpha, RGB or RGBA PNG -> (H,W) or (H,W,C) uint8, with zlib, struct and numpy only
    (rows of filter 0, 1 and 2 without a per-pixel loop).  Anything else raises ValueError."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != _PNG_SIGNATURE:
        raise ValueError("%s is not a PNG file" % path)
    pos, idat, head = 8, [], None
    while pos + 8 <= len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat.append(data)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if head is None:
        raise ValueError("%s has no IHDR chunk" % path)
    w, h, depth, colour, comp, filt, interlace = head
    channels = {0: 1, 4: 2, 2: 3, 6: 4}.get(colour)
    if depth != 8 or channels is None or (comp, filt, interlace) != (0, 0, 0) or w < 1 or h < 1:
        raise ValueError("%s: only non-interlaced 8-bit grey / grey+alpha / RGB / RGBA PNG is read without PIL "
                         "(bit depth %d, colour type %d, interlace %d)" % (path, depth, colour, interlace))
    stride = w * channels
    rows = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if rows.size != h * (1 + stride):
        raise ValueError("%s: %d bytes of image data for %d x %d x %d" % (path, rows.size, h, w, channels))
    rows = rows.reshape(h, 1 + stride)
    if not rows[:, 0].any():                                 # filter 0 throughout: what write_png emits
        out = rows[:, 1:]
    else:
        out = np.zeros((h, stride), np.int64)
        up = np.zeros(stride, np.int64)
        for y in range(h):
            up = out[y] = _unfilter_row(int(rows[y, 0]), rows[y, 1:].astype(np.int64), up, channels)
    out = np.ascontiguousarray(out.astype(np.uint8))
    return out.reshape(h, w) if channels == 1 else out.reshape(h, w, channels)


def read_image(path):
    """an image file -> (H,W,3) uint8 RGB in file row order: grey becomes three channels, a fourth (or grey's second) channel
    is dropped.  PIL when it imports; otherwise `read_png_plain`, and ImportError for what that cannot read."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            if im.mode not in ("L", "LA", "RGB", "RGBA"):
                im = im.convert("RGB")
            a = np.asarray(im, dtype=np.uint8)
    else:
        try:
            a = read_png_plain(path)
        except ValueError as e:
            raise ImportError("reading %s needs PIL (pillow): without it only non-interlaced 8-bit grey / grey+alpha / RGB / "
                              "RGBA PNG files are read (%s)" % (path, e))
    if a.ndim == 2:
        a = np.stack((a,) * 3, -1)
    elif a.shape[2] == 2:
        a = np.stack((a[:, :, 0],) * 3, -1)
    elif a.shape[2] == 4:
        a = a[:, :, :3]
    return np.ascontiguousarray(a)


# ---- the two kernels ---------------------------------------------------------------------------------------------

def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def sample_textures(uv, face_image, face_color, images, texture_size, texture_wrapping='REPEAT', use_bilinear=True, device='cuda'):
    """UV triangles and texture images -> texture cubes (F,ts,ts,ts,3) float32 on the device, one chore_load_textures call
    for all images.  uv (F,3,2), face_image (F) index into `images` or -1 (the face takes its colour), face_color (F,3): arrays
    or tensors; images: a list of (H,W,3) uint8 arrays in file row order."""
    if texture_wrapping not in texture_wrapping_dict:
        raise ValueError("texture_wrapping must be one of %s, got %r" % (sorted(texture_wrapping_dict), texture_wrapping))
    ts = int(texture_size)
    if not 2 <= ts <= 16:
        raise ValueError("texture_size must lie in 2..16, got %r" % (texture_size,))
    dev = _device(device)
    uv_d = torch.as_tensor(uv).detach().to(dev).float().contiguous()
    fi_d = torch.as_tensor(face_image).detach().to(dev).to(torch.int32).contiguous()
    fc_d = torch.as_tensor(face_color).detach().to(dev).float().contiguous()
    Fn = uv_d.shape[0]
    if uv_d.dim() != 3 or tuple(uv_d.shape[1:]) != (3, 2) or Fn < 1 or tuple(fi_d.shape) != (Fn,) or tuple(fc_d.shape) != (Fn, 3):
        raise ValueError("uv (F,3,2), face_image (F) and face_color (F,3) with F >= 1 expected, got %s, %s, %s"
                         % (tuple(uv_d.shape), tuple(fi_d.shape), tuple(fc_d.shape)))
    M = len(images)
    if M > MAX_IMAGES:
        raise ValueError("%d texture images in one call; at most %d" % (M, MAX_IMAGES))
    flat = []
    for a in images:
        a = np.ascontiguousarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
            raise ValueError("a texture image must be a non-empty (H,W,3) uint8 array, got %s %s" % (a.dtype, a.shape))
        flat.append(a)
    offs = np.cumsum([0] + [a.size for a in flat])
    off_c = (ctypes.c_int64 * max(M, 1))(*[int(o) for o in offs[:M]])
    hw_c = (ctypes.c_int * (2 * max(M, 1)))(*[int(s) for a in flat for s in a.shape[:2]])
    img_d = torch.from_numpy(np.concatenate([a.reshape(-1) for a in flat])).to(dev) if M else None
    tex = torch.empty(Fn, ts, ts, ts, 3, dtype=torch.float32, device=dev)
    h = _lib.handle(dev.index)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.chore_load_textures(h, uv_d.data_ptr(), fi_d.data_ptr(), fc_d.data_ptr(),
                                                img_d.data_ptr() if M else None, int(offs[M]), off_c, hw_c, M, Fn, ts,
                                                texture_wrapping_dict[texture_wrapping], 1 if use_bilinear else 0, tex.data_ptr(),
                                                _stream(dev)), h, "chore_load_textures")
    return tex


def atlas_size(num_faces, texture_size_out=16):
    """(height, width) in pixels of the atlas of `num_faces` tiles: integer tile counts, tile_w = isqrt(F-1) + 1"""
    hh, ww = ctypes.c_int(), ctypes.c_int()
    if _lib.lib.chore_texture_atlas_size(int(num_faces), int(texture_size_out), ctypes.byref(hh), ctypes.byref(ww)) != 0:
        raise ValueError("no atlas for %r faces at %r px per tile (F >= 1, texture_size_out >= 2, at most 16384 px on a side)"
                         % (num_faces, texture_size_out))
    return hh.value, ww.value


def texture_atlas(textures, texture_size_out=16):
    """texture cubes (F,ts,ts,ts,3) on the device -> the atlas (H,W,3) float32 on the device, in file row order
    (chore_texture_atlas)"""
    if not torch.is_tensor(textures) or not textures.is_cuda:
        raise RuntimeError("chore_amd needs device tensors (no CPU path)")
    tex = textures.detach().float().contiguous()
    if tex.dim() != 5 or tex.shape[0] < 1 or tex.shape[4] != 3 or not (tex.shape[1] == tex.shape[2] == tex.shape[3]) or \
            not 2 <= tex.shape[1] <= 16:
        raise ValueError("textures (F,ts,ts,ts,3) with F >= 1 and ts in 2..16 expected, got %s" % (tuple(tex.shape),))
    dev = tex.device
    hh, ww = atlas_size(tex.shape[0], texture_size_out)
    image = torch.empty(hh, ww, 3, dtype=torch.float32, device=dev)
    h = _lib.handle(dev.index or 0)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.chore_texture_atlas(h, tex.data_ptr(), tex.shape[0], tex.shape[1], int(texture_size_out), image.data_ptr(),
                                                _stream(dev)), h, "chore_texture_atlas")
    return image


# ---- parsing ---------------------------------------------------------------------------------------------------------

def load_mtl(filename_mtl):
    """colours (Kd) and texture file names (map_Kd) of a .mtl file, by material name  [load_obj.py:13-29]"""
    texture_filenames = {}
    colors = {}
    material_name = ''
    with open(filename_mtl) as f:
        for line in f.readlines():
            words = line.split()
            if not words:
                continue
            if words[0] == 'newmtl':
                material_name = words[1]
            if words[0] == 'map_Kd':
                texture_filenames[material_name] = words[1]
            if words[0] == 'Kd':
                colors[material_name] = np.array(list(map(float, words[1:4])))
    return colors, texture_filenames


def _index(word, what):
    n = int(word)
    if n < 1:
        raise ValueError("relative or zero OBJ %s index %d is not supported" % (what, n))
    return n - 1


def _parse_obj(filename_obj):
    """-> vertices (V,3) float32, faces (F,3) int32, vt (T,2) float32, face_vt (F,3) int32 with -1 where a corner has no vt
    index, one material name per face, the mtllib names in file order.  Polygons are fanned around their first corner."""
    vertices, vts, faces, face_vt, materials, mtllibs = [], [], [], [], [], []
    material_name = ''
    with open(filename_obj) as f:
        lines = f.readlines()
    for line in lines:
        words = line.split()
        if not words:
            continue
        key = words[0]
        if key == 'v':
            vertices.append([float(v) for v in words[1:4]])
        elif key == 'vt':
            vts.append([float(v) for v in words[1:3]])
        elif key == 'usemtl':
            material_name = words[1] if len(words) > 1 else ''
        elif key == 'mtllib' and line.startswith('mtllib') and len(words) > 1:
            mtllibs.append(words[1])
        elif key == 'f':
            corners = []
            for w in words[1:]:
                parts = w.split('/')
                vt = _index(parts[1], "texture") if len(parts) > 1 and parts[1] != '' else -1
                corners.append((_index(parts[0], "vertex"), vt))
            for i in range(len(corners) - 2):
                tri = (corners[0], corners[i + 1], corners[i + 2])
                faces.append([c[0] for c in tri])
                face_vt.append([c[1] for c in tri])
                materials.append(material_name)
    as2d = lambda rows, n, dt: np.asarray(rows, dt).reshape(-1, n)      # noqa: E731
    return as2d(vertices, 3, np.float32), as2d(faces, 3, np.int32), as2d(vts, 2, np.float32), as2d(face_vt, 3, np.int32), \
        materials, mtllibs


def _textures_of(parsed, filename_obj, filename_mtl, texture_size, texture_wrapping, use_bilinear, device):
    _, faces, vts, face_vt, materials, _ = parsed
    if len(faces) < 1:
        raise ValueError("%s has no faces" % filename_obj)
    if face_vt.max() >= len(vts):
        raise ValueError("%s: texture index %d with %d vt lines" % (filename_obj, int(face_vt.max()) + 1, len(vts)))
    colors, texture_filenames = load_mtl(filename_mtl)
    has_uv = (face_vt >= 0).all(axis=1)
    uv = np.zeros((len(faces), 3, 2), np.float32)
    if has_uv.any():
        uv[has_uv] = vts[face_vt[has_uv]]
    face_color = np.full((len(faces), 3), UNKNOWN_MATERIAL_COLOR, np.float32)
    face_image = np.full(len(faces), -1, np.int32)
    names = np.asarray(materials, dtype=object)
    for name, color in colors.items():
        face_color[names == name] = np.asarray(color, np.float32)[:3]
    images, index_of = [], {}
    for name, filename_texture in texture_filenames.items():
        sel = (names == name) & has_uv
        if not sel.any():
            continue
        path = os.path.join(os.path.dirname(filename_obj), filename_texture)
        if path not in index_of:
            index_of[path] = len(images)
            images.append(read_image(path))
        face_image[sel] = index_of[path]
    return sample_textures(uv, face_image, face_color, images, texture_size, texture_wrapping, use_bilinear, device)


def load_textures(filename_obj, filename_mtl, texture_size, texture_wrapping='REPEAT', use_bilinear=True, device='cuda'):
    """the texture cubes (F,ts,ts,ts,3) of an OBJ file's faces, on the device  [load_obj.py:32-106].  Polygons are fanned; a face
    is 0.5 where its material is unknown (or it comes before any `usemtl`), its material's `Kd` where it has one, and sampled
    from the `map_Kd` image where it has one (the image wins over `Kd`).  All materials go through one chore_load_textures call.
    A face with a corner that has no `vt` index, and every face of a file without `vt` lines, stays at its colour (the
    reference takes the file's last `vt`, or raises).  CLAMP_TO_BORDER gives zeros on every textured face, as in the reference.
    Files written by `save_obj` need texture_wrapping='CLAMP_TO_EDGE': the reference's REPEAT sends u = 0 to 1."""
    return _textures_of(_parse_obj(filename_obj), filename_obj, filename_mtl, texture_size, texture_wrapping, use_bilinear, device)


def load_obj(filename_obj, normalization=True, texture_size=4, load_texture=False, texture_wrapping='REPEAT', use_bilinear=True,
             device='cuda'):
    """a Wavefront .obj file -> vertices (V,3) float32, faces (F,3) int32 [, textures (F,ts,ts,ts,3)] on the device
    [load_obj.py:108-164]: `v` and `f` lines, polygons fanned, `normalization` into the cube [-1,1]^3 by the reference's four
    steps.  With load_texture the file's (last) `mtllib` is read through `load_textures`; if none resolves to a file this raises
    the reference's Exception('Failed to load textures.').  Relative (negative) indices raise ValueError.
    Files written by `save_obj` need texture_wrapping='CLAMP_TO_EDGE'."""
    parsed = _parse_obj(filename_obj)
    verts, faces, mtllibs = parsed[0], parsed[1], parsed[5]
    if len(verts) < 1 or len(faces) < 1:
        raise ValueError("%s has no vertices or no faces" % filename_obj)
    if faces.max() >= len(verts):
        raise ValueError("%s: vertex index %d with %d v lines" % (filename_obj, int(faces.max()) + 1, len(verts)))
    dev = _device(device)
    vertices = torch.from_numpy(verts).to(dev)
    faces_d = torch.from_numpy(faces).to(dev)
    textures = None
    if load_texture:
        for name in mtllibs:
            filename_mtl = os.path.join(os.path.dirname(filename_obj), name)
            if os.path.isfile(filename_mtl):
                textures = _textures_of(parsed, filename_obj, filename_mtl, texture_size, texture_wrapping, use_bilinear, dev)
        if textures is None:
            raise Exception('Failed to load textures.')
    if normalization:
        vertices -= vertices.min(0)[0][None, :]
        vertices /= torch.abs(vertices).max()
        vertices *= 2
        vertices -= vertices.max(0)[0][None, :] / 2
    if load_texture:
        return vertices, faces_d, textures
    return vertices, faces_d


# ---- writing ---------------------------------------------------------------------------------------------------------

def atlas_vertices(num_faces, texture_size_out=16):
    """the `vt` coordinates (F,3,2) float32 of the atlas' tile triangles: the tile corner, the corner T px above it and the
    corner T px above and to the right (T = texture_size_out - 1), divided by (W-1, H-1)  [save_obj.py:15-31, integer rows]"""
    hh, ww = atlas_size(num_faces, texture_size_out)
    tile_w = ww // int(texture_size_out)
    fn = np.arange(int(num_faces))
    column, row, tso = fn % tile_w, fn // tile_w, int(texture_size_out)
    v = np.zeros((int(num_faces), 3, 2), np.float32)
    v[:, 0, 0] = column * tso
    v[:, 0, 1] = row * tso
    v[:, 1, 0] = column * tso
    v[:, 1, 1] = (row + 1) * tso - 1
    v[:, 2, 0] = (column + 1) * tso - 1
    v[:, 2, 1] = (row + 1) * tso - 1
    v[:, :, 0] /= np.float32(ww - 1)
    v[:, :, 1] /= np.float32(hh - 1)
    return v


def create_texture_image(textures, texture_size_out=16):
    """texture cubes (F,ts,ts,ts,3) on the device -> (image (H,W,3) float32 numpy in file row order, vertices (F,3,2) float32
    numpy: the `vt` coordinates of every face's tile triangle)  [save_obj.py:10-37].  One tile of texture_size_out px per face,
    isqrt(F-1) + 1 tiles per row; tiles without a face are 0."""
    image = texture_atlas(textures, texture_size_out)
    return image.cpu().numpy(), atlas_vertices(textures.shape[0], texture_size_out)


def _host(x, dtype):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x).astype(dtype)


def save_obj(filename, vertices, faces, textures=None):
    """vertices (V,3) and faces (F,3) [and textures (F,ts,ts,ts,3) on the device] -> `filename` (.obj) and, with textures, the
    .mtl (`newmtl material_1`, `map_Kd`) and .png next to it, in the reference's line formats  [save_obj.py:40-82].  The PNG
    holds round(clip(atlas, 0, 1) * 255).  Such a file loads back with load_obj(..., texture_wrapping='CLAMP_TO_EDGE') only:
    the reference's REPEAT sends u = 0 to 1."""
    verts, tris = _host(vertices, np.float64), _host(faces, np.int64)
    if verts.ndim != 2 or verts.shape[1] != 3 or tris.ndim != 2 or tris.shape[1] != 3:
        raise ValueError("vertices (V,3) and faces (F,3) expected, got %s and %s" % (verts.shape, tris.shape))
    if textures is None:
        return write_obj_files(filename, verts, tris)
    if textures.shape[0] != tris.shape[0]:
        raise ValueError("%d texture cubes for %d faces" % (textures.shape[0], tris.shape[0]))
    texture_image, vertices_textures = create_texture_image(textures)
    write_obj_files(filename, verts, tris, vertices_textures, texture_image)


def write_obj_files(filename, verts, tris, vertices_textures=None, texture_image=None):
    """the host half of `save_obj`: numpy vertices (V,3), faces (F,3) [, `vt` coordinates (F,3,2) and the atlas (H,W,3) float in
    file row order] -> the .obj [, .mtl and .png] files"""
    textured = vertices_textures is not None
    if textured:
        from ..utils.render_utils import write_png
        filename_mtl = filename[:-4] + '.mtl'
        filename_texture = filename[:-4] + '.png'
        material_name = 'material_1'
        write_png(filename_texture, np.round(np.clip(texture_image, 0, 1) * 255).astype(np.uint8))
    out = ['# %s\n' % os.path.basename(filename), '#\n', '\n']
    if textured:
        out.append('mtllib %s\n\n' % os.path.basename(filename_mtl))
    out += ['v %.8f %.8f %.8f\n' % (v[0], v[1], v[2]) for v in np.asarray(verts).tolist()]
    out.append('\n')
    if textured:
        out += ['vt %.8f %.8f\n' % (v[0], v[1]) for v in np.asarray(vertices_textures).reshape((-1, 2)).tolist()]
        out.append('\n')
        out.append('usemtl %s\n' % material_name)
        out += ['f %d/%d %d/%d %d/%d\n' % (f[0] + 1, 3 * i + 1, f[1] + 1, 3 * i + 2, f[2] + 1, 3 * i + 3)
                for i, f in enumerate(np.asarray(tris).tolist())]
        out.append('\n')
    else:
        out += ['f %d %d %d\n' % (f[0] + 1, f[1] + 1, f[2] + 1) for f in np.asarray(tris).tolist()]
    with open(filename, 'w') as f:
        f.write(''.join(out))
    if textured:
        with open(filename_mtl, 'w') as f:
            f.write('newmtl %s\n' % material_name)
            f.write('map_Kd %s\n' % os.path.basename(filename_texture))
