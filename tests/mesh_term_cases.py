"""The cases, inputs, references and the coverage table of tests/test_gpu_mesh_terms.py: the two mesh terms of the fit, the
interpenetration term (csrc/collision.hip) and the silhouette term (csrc/silhouette.hip).  No GPU needed to import this.

A case is a dict with an `id`; CASES maps a family (one GPU test each) to its cases.  The shapes sit around the constants below
(held equal to the sources by tests/test_mesh_term_coverage_table.py): one below, equal to and one above a tile of CT triangles, a
chunk of CHUNK triangles, a block of 256 vertices or doubled faces; sizes that are no multiple of TILE_PX; lists long enough for
the second round of every fixed grid; lists longer than their capacity.  COVERAGE has one row per entry point of chore_amd/_lib.py
that starts with chore_collision_, chore_silhouette_ or chore_sil_project_.  Inputs and references are built once per case
(functools.lru_cache) and must not be written to."""
import functools
import zlib

import numpy as np
import torch

import collision_ref as cr
from meshes import icosphere
from oracle import silhouette as osil

FAMILIES = ("chore_collision_", "chore_silhouette_", "chore_sil_project_")
CONSTANTS = {
    "CT": 128,                      # collision.hip: triangles per tile side of the broad phase
    "CAND_CAP": (24, 4096),         # collision.hip: cand_cap = 24 F + 4096
    "PAIR_CAP": (8, 1024),          # collision.hip: pair_cap = 8 F + 1024
    "BROAD_GRID": 1024,             # coll_broad_kernel: workgroups per frame, each takes tile pairs g, g + 1024, ...
    "NARROW_THREADS": 256 * 256,    # coll_narrow_kernel: threads per frame of its fixed grid
    "LOSS_THREADS": 256 * 64,       # coll_loss_kernel: threads per frame of its fixed grid
    "TILEPAIR_BLOCK": 256,          # coll_tilepairs_kernel: tile pairs per workgroup
    "CHUNK": 256,                   # silhouette.hip: triangles per LDS chunk of sil_fwd_kernel
    "TILE_PX": 16,                  # silhouette.hip: pixels per tile side
    "PROJ_BLOCK": 256,              # silhouette.hip: doubled faces per workgroup (forward), vertices per loop round (backward)
}
CT, CHUNK = CONSTANTS["CT"], CONSTANTS["CHUNK"]
GRAZE = 1e-4                        # a candidate pair whose |SAT margin| is below this is taken out of a soup
MIN_ANGLE = 15.0                    # a soup triangle whose smallest angle is below this is redrawn
SOUP_CHURN_CAP = 0.02               # at most this fraction of a case's triangles is redrawn or removed
DIST5 = (0.1, -0.05, 0.01, -0.02, 0.03)


def cand_cap(F):
    return CONSTANTS["CAND_CAP"][0] * F + CONSTANTS["CAND_CAP"][1]


def pair_cap(F):
    return CONSTANTS["PAIR_CAP"][0] * F + CONSTANTS["PAIR_CAP"][1]


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


CASES = {}


def _add(family, name, **kw):
    CASES.setdefault(family, []).append(dict(kw, id="%s.%s" % (family, name), family=family))


def ids(family):
    return [c["id"] for c in CASES[family]]


def case(cid):
    return next(c for cs in CASES.values() for c in cs if c["id"] == cid)


# ====================================================================================================== triangle soups
def min_angle(t):
    t = np.asarray(t, np.float64)
    out = []
    for k in range(3):
        a, b = t[:, (k + 1) % 3] - t[:, k], t[:, (k + 2) % 3] - t[:, k]
        c = (a * b).sum(-1) / np.sqrt((a * a).sum(-1) * (b * b).sum(-1))
        out.append(np.degrees(np.arccos(np.clip(c, -1, 1))))
    return np.min(out, 0)


def _draw(rs, n, box, scale):
    """n triangles, each with its own three corners: a seeded centre in [0, box]^3, a random plane, corners at 0 / 120 / 240 degrees
    (+- 25) and 0.6 ... 1 x scale from the centre"""
    c = rs.uniform(0, box, (n, 1, 3))
    q, _ = np.linalg.qr(rs.standard_normal((n, 3, 3)))
    ang = np.radians(np.array([0.0, 120.0, 240.0]) + rs.uniform(-25, 25, (n, 3)))
    rad = scale * rs.uniform(0.6, 1.0, (n, 3))
    off = rad[..., None] * (np.cos(ang)[..., None] * q[:, None, :, 0] + np.sin(ang)[..., None] * q[:, None, :, 1])
    return (c + off).astype(np.float32)


@functools.lru_cache(maxsize=None)
def soup(seed, F, box, scale):
    """-> (triangles (F,3,3) float32, number redrawn + removed).  Consecutive triangles are unrelated, so every tile's box is the
    whole box.  Triangles with a smallest angle below MIN_ANGLE are redrawn; triangles of a candidate pair whose SAT margin is
    below GRAZE are removed (fp32 and float64 then decide every remaining pair alike); F is the count after that."""
    rs = np.random.RandomState(seed)
    n0 = F + max(4, F // 50)
    t = _draw(rs, n0, box, scale)
    churn = 0
    while True:
        bad = np.nonzero(min_angle(t) < MIN_ANGLE)[0]
        if not len(bad):
            break
        churn += len(bad)
        t[bad] = _draw(rs, len(bad), box, scale)
    _, cand, m = cr.find_pairs(t.reshape(-1, 3), np.arange(3 * n0).reshape(-1, 3), True)
    drop = np.unique(cand[np.abs(m) < GRAZE].ravel())
    keep = np.setdiff1d(np.arange(n0), drop)
    assert len(keep) >= F, (seed, F, len(keep))
    t = np.ascontiguousarray(t[keep[:F]])
    t.setflags(write=False)
    return t, churn + len(drop)


def _soup_mesh(frames):
    """list of (F,3,3) triangle arrays -> verts (B, 3F, 3) float32, faces (F,3) int32 (every triangle its own three vertices)"""
    F = len(frames[0])
    return np.stack([t.reshape(-1, 3) for t in frames]).astype(np.float32), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def _crossing(seed, apart):
    """two triangles that cross (or, `apart`, that do not)"""
    rs = np.random.RandomState(seed)
    t = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0.25, 0.25, -0.5], [0.3, 0.2, 0.5], [0.7, 0.6, 0.1]]], np.float64)
    t += rs.uniform(-0.03, 0.03, t.shape)
    if apart:
        t[1] += 5.0
    return t.astype(np.float32)


# density of the tile-edge soups: box 1, corner scale by F (at least F / 4 pairs per frame, held by the CPU suite)
_TILE_SCALE = {127: 0.2, 128: 0.2, 129: 0.2, 257: 0.15}
SPREAD_BOX = 60.0            # the middle frame of a B = 3 case: the same triangles' sizes in a box where none meets another


def _tile_frames(F, B):
    out = []
    for b in range(B):
        spread = B == 3 and b == 1
        if F == 1:
            out.append(_draw(np.random.RandomState(_seed("one", b)), 1, 1.0, 0.3))
        elif F == 2:
            out.append(_crossing(_seed("two", b), spread))
        else:
            out.append(soup(_seed("tile", F, b), F, SPREAD_BOX if spread else 1.0, _TILE_SCALE[F])[0])
    return out


for _F in (1, 2, CT - 1, CT, CT + 1, 2 * CT + 1):
    for _B in (1, 3):
        _add("coll_tiles", "F%d.B%d" % (_F, _B), F=_F, B=_B, kind="tiles")
# the second round of every fixed grid: nt = 45 tiles -> 1035 tile pairs > 1024 workgroups of the broad phase and > 256 threads of
# the tile-pair kernel; more candidates than the narrow phase has threads, more pairs than the loss kernel has threads
ROUNDS = dict(F=5755, seed=_seed("rounds"), box=1.0, scale=0.095)
_add("coll_rounds", "F%d" % ROUNDS["F"], F=ROUNDS["F"], B=1, kind="rounds")
_add("coll_meshes", "spheres", kind="spheres", B=2)
_add("coll_meshes", "spheres_seam", kind="spheres_seam", B=2)
_add("coll_order", "soup257", kind="perm", of="coll_tiles.F257.B3")
_add("coll_order", "spheres", kind="perm", of="coll_meshes.spheres")
_add("coll_order", "rounds", kind="perm", of="coll_rounds.F%d" % ROUNDS["F"])
_add("coll_zero_area", "F129", kind="zero_area", of="coll_tiles.F129.B1")
_add("coll_caps", "m64", kind="caps", m=64, B=1, counts=[2048, 0, 2048])
_add("coll_caps", "m100", kind="caps", m=100, B=1, counts=[2624, 1104, 6272])


def two_spheres():
    """the two icospheres of tests/test_gpu_collision.py (F = 320 + 320, two frames)"""
    va, fa = icosphere(2, 1.0)
    vb, fb = icosphere(2, 0.55, (1.25, 0.13, -0.07))
    va32, vb32 = va.astype(np.float32), vb.astype(np.float32)
    verts = np.concatenate([np.stack([va32, va32]), np.stack([vb32, vb32 + np.float32([0.1, 0.0, 0.05])])], 1)
    return verts, np.concatenate([fa, fb + len(va)], 0).astype(np.int32), len(va)


def seam(verts, faces, nA):
    """duplicate the vertices of the larger sphere's ring |z| < 0.1: its faces above the ring use the copies (appended at the end),
    the faces below keep the originals -- equal positions, different indices along the seam.  -> verts, faces, ring, copies"""
    ring = np.nonzero(np.abs(verts[0, :nA, 2]) < 0.1)[0]
    V = verts.shape[1]
    copy_of = np.arange(V)
    copy_of[ring] = V + np.arange(len(ring))
    f = faces.copy()
    upper = np.nonzero((verts[0][faces].mean(1)[:, 2] > 0) & (faces.max(1) < nA))[0]
    f[upper] = copy_of[faces[upper]]
    return np.concatenate([verts, verts[:, ring]], 1), f.astype(np.int32), ring, copy_of[ring]


def caps_grid(m):
    """m horizontal triangles at distinct heights, then m vertical ones at distinct x: every vertical crosses every horizontal, no
    two of a kind have overlapping boxes -> exactly m^2 candidates, all of them pairs.  Three more vertices belong to no face."""
    t = np.zeros((2 * m, 3, 3), np.float64)
    for k in range(m):
        z = (k + 0.5) / m
        t[k] = [[-1, -1, z], [3, -1, z], [-1, 3, z]]
        x = (k + 0.5) / m
        t[m + k] = [[x, 0.2, -1], [x, 0.8, -1], [x, 0.5, 2]]
    verts = np.concatenate([t.reshape(-1, 3), [[9, 9, 9], [9, 8, 9], [8, 9, 9]]], 0).astype(np.float32)[None]
    return verts, np.arange(6 * m, dtype=np.int32).reshape(2 * m, 3)


def zero_area_triangle(tris):
    """three distinct collinear corners on a line along x (both edge vectors are (dx, 0, 0): the cross product is exactly 0 in any
    precision) through the centroid of soup triangle 0, whose plane the line crosses"""
    c = tris[0].astype(np.float64).mean(0)
    return np.float32([[c[0] - 0.125, c[1], c[2]], [c[0], c[1], c[2]], [c[0] + 0.125, c[1], c[2]]])


@functools.lru_cache(maxsize=None)
def collision_inputs(cid):
    """-> verts (B,V,3) float32, faces (F,3) int32"""
    c = case(cid)
    if c["kind"] == "tiles":
        v, f = _soup_mesh(_tile_frames(c["F"], c["B"]))
    elif c["kind"] == "rounds":
        v, f = _soup_mesh([soup(ROUNDS["seed"], ROUNDS["F"], ROUNDS["box"], ROUNDS["scale"])[0]])
    elif c["kind"] == "spheres":
        v, f, _ = two_spheres()
    elif c["kind"] == "spheres_seam":
        v, f, _, _ = seam(*two_spheres())
    elif c["kind"] == "perm":
        v, f = collision_inputs(c["of"])
        f = f[np.random.RandomState(_seed("perm", cid)).permutation(len(f))]
    elif c["kind"] == "zero_area":
        v, f = collision_inputs(c["of"])
        v = np.concatenate([v, zero_area_triangle(v[0][f[0]].reshape(1, 3, 3))[None]], 1)
        f = np.concatenate([f, [[v.shape[1] - 3, v.shape[1] - 2, v.shape[1] - 1]]], 0).astype(np.int32)
    elif c["kind"] == "caps":
        v, f = caps_grid(c["m"])
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def soup_churn(cid):
    """triangles redrawn or removed while the case's soups were built, per frame"""
    c = case(cid)
    if c["kind"] == "rounds":
        return [soup(ROUNDS["seed"], ROUNDS["F"], ROUNDS["box"], ROUNDS["scale"])[1]]
    if c["kind"] == "tiles" and c["F"] > 2:
        return [soup(_seed("tile", c["F"], b), c["F"], SPREAD_BOX if (c["B"] == 3 and b == 1) else 1.0, _TILE_SCALE[c["F"]])[1]
                for b in range(c["B"])]
    return []


@functools.lru_cache(maxsize=None)
def collision_reference(cid):
    """per frame: dict(pairs (P,2), loss, per (P,) pair losses, grad (V,3), e32_loss, e32_grad (V,3) |float32 - float64|, n (V,))"""
    v, f = collision_inputs(cid)
    out = []
    for b in range(v.shape[0]):
        pairs = cr.find_pairs(v[b], f)
        loss, per, grad = cr.loss_and_grad(v[b], f, pairs, torch.float64)
        loss32, _, grad32 = cr.loss_and_grad(v[b], f, pairs, torch.float32)
        out.append(dict(pairs=pairs, loss=loss, per=per, grad=grad, e32_loss=abs(loss32 - loss), e32_grad=np.abs(grad32 - grad),
                        n=cr.touches(f, pairs, v.shape[1])))
    return out


# ====================================================================================================== silhouette lists
# (L, size, B) and the half-width of a triangle in pixels; the lists of the backward cases keep their triangles near 10 px so that
# the oracle's scalar edge walk takes seconds
_SIL = [(1, 15, 1, 5.0), (255, 16, 1, 2.5), (256, 17, 3, 4.0), (257, 50, 1, 5.0), (600, 50, 3, 4.0), (600, 17, 1, 2.5)]
REPEAT_SRC, REPEAT_AT = 3, 300      # lists that reach index 300 repeat triangle 3 there: same depth everywhere, the smaller index wins
for _L, _S, _B, _h in _SIL:
    _add("sil_fwd", "L%d.S%d.B%d" % (_L, _S, _B), L=_L, size=_S, B=_B, half=_h)
for _L, _S, _B, _h in _SIL[2:4]:
    _add("sil_bwd", "L%d.S%d.B%d" % (_L, _S, _B), L=_L, size=_S, B=_B, half=_h, fwd="sil_fwd.L%d.S%d.B%d" % (_L, _S, _B))


def _front(t):
    """make a triangle front-facing (swap two corners of a culled one)"""
    f = t.reshape(9)
    if (f[7] - f[1]) * (f[3] - f[0]) < (f[4] - f[1]) * (f[6] - f[0]):
        t[[1, 2]] = t[[2, 1]]
    return t


@functools.lru_cache(maxsize=None)
def sil_triangles(L, size, B, half):
    """(B,L,3,3) float32 projected triangles of both windings: a centre in the view, corner offsets of +- `half` pixels, a depth
    per corner.  Crafted: a list of one triangle is front-facing; the only triangle of a last chunk (index 256 of 257) is front-facing,
    three times as large and at mid depth, so that it wins some pixels and loses others; triangle 3 of a list that reaches index
    300 is front-facing, twice as large, nearer the centre and in front of everything, and index 300 repeats it."""
    rs = np.random.RandomState(_seed("sil", L, size, B))
    h = 2.0 * half / size
    c = rs.uniform(-1.0, 1.0, (B, L, 1, 2))
    xy = c + rs.uniform(-h, h, (B, L, 3, 2))
    z = rs.uniform(0.5, 4.0, (B, L, 3, 1))
    t = np.concatenate([xy, z], -1).astype(np.float32)
    for b in range(B):
        if L == 1:
            t[b, 0] = _front(t[b, 0])
        if L == CHUNK + 1:
            t[b, CHUNK, :, :2] = np.float32([0.1, -0.05]) + 3 * (t[b, CHUNK, :, :2] - c[b, CHUNK])
            t[b, CHUNK, :, 2] = 1.6
            t[b, CHUNK] = _front(t[b, CHUNK])
        if L > REPEAT_AT:
            t[b, REPEAT_SRC, :, :2] = c[b, REPEAT_SRC] * 0.5 + 2 * (t[b, REPEAT_SRC, :, :2] - c[b, REPEAT_SRC])
            t[b, REPEAT_SRC, :, 2] = 0.45
            t[b, REPEAT_SRC] = _front(t[b, REPEAT_SRC])
            t[b, REPEAT_AT] = t[b, REPEAT_SRC]
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def sil_reference(cid):
    """-> triangles, face_index, alpha of oracle/silhouette.rasterize_fwd"""
    c = case(cid)
    t = sil_triangles(c["L"], c["size"], c["B"], c["half"])
    fim, alpha = osil.rasterize_fwd(t, c["size"])
    return t, fim, alpha


@functools.lru_cache(maxsize=None)
def sil_bwd_reference(cid):
    """-> triangles, face_index, alpha, upstream gradient, oracle/silhouette.rasterize_bwd (B,L,3,3)"""
    c = case(cid)
    t, fim, alpha = sil_reference(c["fwd"])
    g = np.random.RandomState(_seed("silg", cid)).standard_normal(alpha.shape).astype(np.float32)
    return t, fim, alpha, g, osil.rasterize_bwd(t, fim, alpha, g)


# ====================================================================================================== projection
_PROJ = [  # V, F, B, distortion, orig_size, cam_broadcast
    (3, 1, 1, 0, 1, 1), (3, 1, 1, 1, 1, 0), (3, 1, 3, 1, 2, 0),
    (255, 127, 1, 1, 1, 1), (255, 127, 3, 0, 2, 0),
    (256, 128, 1, 1, 2, 1), (256, 128, 3, 1, 1, 0),
    (257, 129, 1, 0, 2, 1), (257, 129, 3, 1, 1, 0), (257, 129, 3, 1, 2, 1),
    (600, 1100, 1, 1, 1, 1), (600, 1100, 3, 1, 2, 0), (600, 1100, 3, 0, 1, 1),
]
for _V, _F, _B, _d, _o, _bc in _PROJ:
    _add("sil_project", "V%d.F%d.B%d.%s.orig%d.%s" % (_V, _F, _B, "dist" if _d else "plain", _o, "bcast" if _bc else "percam"),
         V=_V, F=_F, B=_B, dist=_d, orig=float(_o), bcast=_bc)


def corner_adjacency(faces, V):
    """per vertex the entries (f2 * 3 + corner) of the doubled face list (faces, then reversed corners), ascending"""
    f = np.asarray(faces, np.int64)
    both = np.concatenate([f, f[:, ::-1]], 0).reshape(-1)
    off = np.zeros(V + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(both, minlength=V))
    return off.astype(np.int32), np.argsort(both, kind="stable").astype(np.int32)


def _rotation(rs):
    """a camera rotation near the identity (Q of a QR with the signs of R's diagonal taken out)"""
    q, r = np.linalg.qr(np.eye(3) + 0.1 * rs.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))[None]


@functools.lru_cache(maxsize=None)
def project_inputs(cid):
    c = case(cid)
    V, F, B = c["V"], c["F"], c["B"]
    rs = np.random.RandomState(_seed("proj", V, F, B, c["dist"], c["orig"], c["bcast"]))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731
    verts = f32(rs.uniform(-0.6, 0.6, (B, V, 3)))
    faces = np.arange(3)[None] if F == 1 else np.stack([rs.choice(V, 3, replace=False) for _ in range(F)])
    nc = 1 if c["bcast"] else B
    K = np.array([[1.6, 0.02, 0.5], [0.01, 1.5, 0.48], [0, 0, 1]]) * c["orig"] + rs.uniform(-0.02, 0.02, (B, 3, 3))
    K[:, 2] = [0, 0, 1]
    off, ent = corner_adjacency(faces, V)
    d = dict(verts=verts, faces=np.ascontiguousarray(np.stack([faces] * B), np.int32),
             Ro=f32(np.eye(3) + 0.2 * rs.standard_normal((B, 3, 3))), to=f32(np.concatenate([rs.uniform(-0.1, 0.1, (B, 2)), rs.uniform(2.0, 3.0, (B, 1))], 1)),
             s=f32(rs.uniform(0.8, 1.2, B)), K=f32(K),
             cam_R=f32(np.stack([_rotation(rs) for _ in range(nc)])),
             cam_t=f32(rs.uniform(-0.05, 0.1, (nc, 3))), g=f32(rs.standard_normal((B, 2 * F, 3, 3))), adj_off=off, adj=ent,
             dist5=np.float32(DIST5) if c["dist"] else None, orig=c["orig"], eps=1e-9)
    return d


def project_ref(d, dtype):
    """apply_transformation -> projection(dist_coeffs, orig_size) -> vertices_to_faces with both windings, as torch expressions in
    `dtype` on the CPU; autograd for the seeded upstream gradient.  -> tri (B,2F,3,3), dRo, dto, ds as float64 numpy"""
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)      # noqa: E731
    verts, K, Rc, tc, g = T(d["verts"]), T(d["K"]), T(d["cam_R"]), T(d["cam_t"]), T(d["g"])
    Ro, to, s = (T(d[k]).requires_grad_(True) for k in ("Ro", "to", "s"))
    B = verts.shape[0]
    w = s.view(-1, 1, 1) * (torch.bmm(verts, Ro) + to.unsqueeze(1))                    # apply_transformation
    v = torch.matmul(w, Rc.transpose(2, 1)) + tc.unsqueeze(1)                           # projection
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    x_, y_ = x / (z + d["eps"]), y / (z + d["eps"])
    k1, k2, p1, p2, k3 = (float(np.float32(q)) for q in (d["dist5"] if d["dist5"] is not None else np.zeros(5)))
    r2 = x_ ** 2 + y_ ** 2
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x_ * rad + 2 * p1 * x_ * y_ + p2 * (r2 + 2 * x_ ** 2)
    yd = y_ * rad + p1 * (r2 + 2 * y_ ** 2) + 2 * p2 * x_ * y_
    uv = torch.matmul(torch.stack([xd, yd, torch.ones_like(z)], -1), K.transpose(1, 2))
    o = d["orig"]
    u, vv = uv[..., 0], o - uv[..., 1]
    pv = torch.stack([2 * (u - o / 2.0) / o, 2 * (vv - o / 2.0) / o, z], -1)
    f = torch.as_tensor(d["faces"].astype(np.int64))
    f2 = torch.cat([f, f.flip(-1)], 1)                                                  # fill_back
    tri = torch.stack([pv[b][f2[b]] for b in range(B)])                                 # vertices_to_faces
    (tri * g).sum().backward()
    return tuple(a.detach().double().numpy() for a in (tri, Ro.grad, to.grad, s.grad))


@functools.lru_cache(maxsize=None)
def project_reference(cid):
    """-> (float64 results, E32 per result = largest |float32 - float64|)"""
    d = project_inputs(cid)
    r64, r32 = project_ref(d, torch.float64), project_ref(d, torch.float32)
    return r64, tuple(float(np.abs(a - b).max()) for a, b in zip(r32, r64))


# ====================================================================================================== coverage
_ALL_COLL = [i for fam in ("coll_tiles", "coll_rounds", "coll_meshes", "coll_order", "coll_zero_area", "coll_caps") for i in ids(fam)]
COVERAGE = {
    "chore_collision_workspace_bytes": _ALL_COLL,
    "chore_collision_fwd": _ALL_COLL,
    "chore_collision_bwd": ids("coll_tiles"),
    "chore_silhouette_workspace_bytes": ids("sil_fwd") + ids("sil_bwd"),
    "chore_silhouette_fwd": ids("sil_fwd") + ids("sil_bwd"),
    "chore_silhouette_bwd": ids("sil_bwd"),
    "chore_sil_project_fwd": ids("sil_project"),
    "chore_sil_project_bwd": ids("sil_project"),
}
