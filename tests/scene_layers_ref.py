"""numpy float32 restatement of steps 2-8 of chore_scene_layers_fwd's rule (include/chore_hip.h) on GIVEN per-sample layers,
in the style of tests/scene_ref.py, whose `resolve` serves here too.  It decides nothing about coverage: every face layer
holds, per sample, the face that a set of faces shows there (hand-made, or chore_render_fwd's output at ssaa = 1 on those faces
alone, which is that set's candidate with the smallest depth, then the smallest index), and the point layer is
chore_splat_fwd's.  What is restated is the grouping of the layers, their order, the cut at K, which of them lie before the
point, the cut at an opaque face, the blend, the alpha fold and the ids.  Every operation is one numpy operation on float32
values in the association the header writes down.
"""
import numpy as np

from scene_ref import resolve  # noqa: F401  (the resolve of the layered rule is chore_scene_fwd's)

F32 = np.float32


def listed(face_id, zf, layers, group=None):
    """steps 2 and 3.  face_id (G,) + X int (-1 = none), zf (G,) + X; group (G,) ints or None = every layer its own group.
    -> order (G,) + X: the layers of every sample by (zf, face_id) ascending with the unlisted ones last, and n X: how many
    are listed (at most `layers`), and survivors X: how many there were before the cut at `layers`"""
    face_id, zf = np.asarray(face_id), np.asarray(zf, F32)
    G = face_id.shape[0]
    alive = face_id >= 0
    if group is not None:
        group = np.asarray(group)
        for a in range(G):
            for b in range(a + 1, G):
                if group[a] != group[b]:
                    continue
                both = alive[a] & alive[b]
                a_wins = (zf[a] < zf[b]) | ((zf[a] == zf[b]) & (face_id[a] < face_id[b]))
                alive[b] = alive[b] & ~(both & a_wins)
                alive[a] = alive[a] & ~(both & ~a_wins)
    order = np.lexsort((face_id, zf, ~alive), axis=0)              # the last key counts first
    survivors = alive.sum(axis=0)
    return order, np.minimum(survivors, int(layers)), survivors


def structure(face_id, zf, opacity, layers, point_id, zn, bias, group=None):
    """steps 2-6 -> order (G,)+X, o (G,)+X clamped opacities in that order, n X listed, j X before the point, v X visible,
    survivors X"""
    face_id, zf = np.asarray(face_id), np.asarray(zf, F32)
    G = face_id.shape[0]
    order, n, survivors = listed(face_id, zf, layers, group)
    z = np.take_along_axis(zf, order, axis=0)
    if opacity is None:
        o = np.ones(zf.shape, F32)
    else:
        o = np.take_along_axis(np.asarray(opacity, F32), order, axis=0)
        with np.errstate(all="ignore"):
            o = np.where(np.isnan(o), F32(0), np.minimum(np.maximum(o, F32(0)), F32(1))).astype(F32)
    rank = np.arange(G).reshape((G,) + (1,) * (zf.ndim - 1))
    point = np.asarray(point_id) >= 0
    with np.errstate(all="ignore"):
        behind = point[None] & ((np.asarray(zn, F32) - F32(bias)).astype(F32)[None] < z)      # equality goes to the face
    before = (rank < n[None]) & ~behind
    j = before.sum(axis=0)
    assert np.array_equal(before, rank < j[None]), "depths ascend, so the faces before the point are a prefix"
    opaque = before & (o >= F32(1))
    v = np.where(opaque.any(axis=0), opaque.argmax(axis=0) + 1, j)
    return order, o, n, j, v, survivors


def compose(face_id, m, zf, opacity, layers, point_id, p, zn, bias, background, far, group=None):
    """face_id (G,)+X int (-1 = none), m (G,)+X+(3,) face colours, zf (G,)+X depths, opacity (G,)+X (each layer's face's,
    unclamped; ignored without a face) or None = 1, layers = K, group (G,) or None; point_id X int (-1 = none), p X+(3,) shaded
    point colour, zn X point depth; bias, far scalars; background (3,).
    -> colour X+(3,), depth X, alpha X float32 and id X int32 (f a face, -2 - n a point, -1 nothing)"""
    face_id, point_id = np.asarray(face_id), np.asarray(point_id)
    m, zf, p, zn = (np.asarray(a, F32) for a in (m, zf, p, zn))
    G = face_id.shape[0]
    order, o, n, j, v, _ = structure(face_id, zf, opacity, layers, point_id, zn, bias, group)
    f = np.take_along_axis(face_id, order, axis=0)
    z = np.take_along_axis(zf, order, axis=0)
    col = np.take_along_axis(m, order[..., None], axis=0)
    point = point_id >= 0
    bg = np.asarray(background, F32)
    under = np.where(point[..., None], p, bg).astype(F32)
    c, a = under, np.zeros(point.shape, F32)
    for i in range(G - 1, -1, -1):                                   # i = v down to 1
        on = i < v
        one_minus = (F32(1) - o[i]).astype(F32)
        blend = ((o[i][..., None] * col[i]).astype(F32) + (one_minus[..., None] * c).astype(F32)).astype(F32)
        c = np.where(on[..., None], np.where((o[i] >= F32(1))[..., None], col[i], blend), c).astype(F32)
        a = np.where(on, (o[i] + (one_minus * a).astype(F32)).astype(F32), a).astype(F32)
    face = v >= 1
    last = np.take_along_axis(o, np.maximum(v - 1, 0)[None], axis=0)[0]
    colour = np.where(face[..., None], c, under).astype(F32)
    depth = np.where(face, z[0], np.where(point, zn, F32(far))).astype(F32)
    alpha = np.where(face, np.where(point | (last >= F32(1)), F32(1), a), np.where(point, F32(1), F32(0))).astype(F32)
    ident = np.where(face, f[0], np.where(point, -2 - point_id, -1)).astype(np.int32)
    return colour, depth, alpha, ident
