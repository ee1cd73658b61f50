"""numpy float32 restatement of the composite rule of chore_scene_fwd (include/chore_hip.h) on GIVEN per-sample layers, plus
the resolve.  It decides nothing about coverage: the face layer and the point layer come from elsewhere (hand-made, or the
outputs of chore_render_fwd / chore_splat_fwd at ssaa = 1, where a pixel is one sample), so what is restated here is only
which layer is in front, the blend under a translucent face, and the ids.  Every operation is one numpy operation on float32
values in the association the header writes down.
"""
import numpy as np

import render_ref

F32 = np.float32


def compose(face_id, m, zf, point_id, p, zn, opacity, bias, background, far):
    """per sample (any leading shape X): face_id X int (-1 = none), m X+(3,) face colour, zf X face depth; point_id X int
    (-1 = none), p X+(3,) shaded point colour, zn X point depth; opacity X (the winning face's, unclamped; ignored without a
    face) or None = 1; bias, far scalars; background (3,).
    -> colour X+(3,), depth X, alpha X float32 and id X int32 (f a face, -2 - n a point, -1 nothing)"""
    face_id, point_id = np.asarray(face_id), np.asarray(point_id)
    m, zf, p, zn = (np.asarray(a, F32) for a in (m, zf, p, zn))
    bias, far, bg = F32(bias), F32(far), np.asarray(background, F32)
    face, point = face_id >= 0, point_id >= 0
    with np.errstate(all="ignore"):
        if opacity is None:
            o = np.ones(face_id.shape, F32)
        else:
            o = np.asarray(opacity, F32)
            o = np.where(np.isnan(o), F32(0), np.minimum(np.maximum(o, F32(0)), F32(1))).astype(F32)
        front = point & (~face | ((zn - bias) < zf))                      # equality goes to the face
        under = np.where(point[..., None], p, bg)
        one_minus = (F32(1) - o).astype(F32)
        blend = ((o[..., None] * m).astype(F32) + (one_minus[..., None] * under).astype(F32)).astype(F32)
        face_colour = np.where((o >= F32(1))[..., None], m, blend)
    colour = np.where(front[..., None], p, np.where(face[..., None], face_colour, bg)).astype(F32)
    depth = np.where(front, zn, np.where(face, zf, far)).astype(F32)
    alpha = np.where(front, F32(1), np.where(face, np.where(point, F32(1), o), F32(0))).astype(F32)
    ident = np.where(front, -2 - point_id, np.where(face, face_id, -1)).astype(np.int32)
    return colour, depth, alpha, ident


def resolve(colour, depth, alpha, ssaa):
    """per-sample images, rows not flipped (B,S,S,3), (B,S,S), (B,S,S) -> rgb (B,3,size,size), depth, alpha (B,size,size): the
    order of tests/render_ref.py's resolve, which is the kernels'"""
    return render_ref.resolve(np.asarray(colour, F32), np.asarray(depth, F32), np.asarray(alpha, F32), ssaa)
