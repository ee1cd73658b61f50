"""GPU: the gradient of the mesh distance (chore_mesh_dist_bwd, csrc/mesh_dist_bwd.hip, through
chore_amd.preprocess.mesh_distance) against the float64 restatement in tests/mesh_grad_ref.py.

The bound of every comparison is 8 x E32, E32 = the largest |float32 - float64| of the restatement itself on the case's own
kept points, taken separately for dpoints and dverts (computed here once per run and asserted to lie in (0, 1e-2)).  Points
where two triangles with different closest points tie (mesh_grad_ref.ties, at most 1 % of a case) are left out by giving them
the upstream gradient 0: they then contribute exactly 0 to both outputs.

Shapes: the forward's point tile is 512 points.  The backward's point pass has 256 threads; its gather pass gives one vertex
to each of 256 threads (one vertex tile = 256), streams the point records through LDS in tiles of 256 and splits the points
into S = min(ceil(2048 / (B * vertex tiles)), ceil(N / 256), 64) chunks (mb_chunks).  So: N = 1, 255 (S = 1); 257, 511 (S = 2,
the second chunk one point / one short of full); 513, 600 (S = 3); N = 16 385 (65 record tiles: S at its cap of 64, chunks of
two tiles, the 33rd holds one point and 31 are empty).  V = 8 (box12), 162 (ico2), 255 and 257 (ico2's vertices scattered over
255 / 257 slots, the rest unreferenced: one tile short of full, a second tile with one vertex), 866 (box1728: 4 tiles),
6 890 (body: 27 tiles).  B = 1 and B = 3 with a different mesh per frame."""
import numpy as np
import pytest
import torch

import mesh_grad_ref as gref
from mesh_grad_ref import f32

pytestmark = pytest.mark.gpu

NAMES = ("box12", "box1728", "ico2", "hemi", "body")


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def gpu_grads(P, V, F, g, dp=True, dv=True, want="dist", **kw):
    """d (sum_i g_i out_i) / d points, / d verts through mesh_distance -> (out, dpoints or None, dverts or None) as numpy"""
    from chore_amd.preprocess import mesh_distance
    p, v = dev(P, np.float32).requires_grad_(dp), dev(V, np.float32).requires_grad_(dv)
    out = mesh_distance(p, v, dev(F, np.int32), want, **kw)
    out.backward(dev(g, np.float32))
    return (out.detach().cpu().numpy(), None if p.grad is None else p.grad.cpu().numpy(), None if v.grad is None else v.grad.cpu().numpy())


@pytest.fixture(scope="module")
def cases():
    """meshes, points, upstream gradients and the float64 / float32 restatement of every case, computed once, left unchanged"""
    c = {n: gref.make_case(n) for n in NAMES}
    assert [len(c[k]["F"]) for k in NAMES] == [12, 1728, 320, 152, 13776]
    assert [len(c[k]["V"]) for k in NAMES] == [8, 866, 162, 162, 6890]
    assert [len(c[k]["P"]) for k in NAMES] == [600, 600, 600, 600, 513]
    for k in NAMES:
        assert c[k]["tie"].sum() <= gref.TIE_CAP * len(c[k]["P"])
        for e in ("E32_dP", "E32_dV", "E32_dP_sharp", "E32_dV_sharp"):
            assert 0 < c[k][e] < 1e-2, (k, e, c[k][e])
    return c


def compare(what, P, V, F, g, r64=None, E=None):
    """dpoints and dverts of the kernel within 8 E32 of the float64 restatement; E32 measured here unless given"""
    if r64 is None:
        r64, eP, eV = gref._e32(P, V, F, g)
    else:
        eP, eV = E
    assert 0 < eP < 1e-2 and 0 < eV < 1e-2, (what, eP, eV)
    _, dP, dV = gpu_grads(P, V, F, g)
    assert dP.shape == P.shape and dV.shape == V.shape and dP.dtype == dV.dtype == np.float32
    errP, errV = np.abs(dP - r64["dP"]).max(), np.abs(dV - r64["dV"]).max()
    print("%s: dpoints E32 %.3e  kernel %.3e (%.2f E32);  dverts E32 %.3e  kernel %.3e (%.2f E32)"
          % (what, eP, errP, errP / eP, eV, errV, errV / eV))
    assert np.isfinite(dP).all() and np.isfinite(dV).all()
    assert errP <= 8 * eP, (what, errP, 8 * eP)
    assert errV <= 8 * eV, (what, errV, 8 * eV)
    return dP, dV


@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_float64(cases, name):
    """1: every case on its kept points, and the sharper comparison on the points at least 1e-2 from the surface"""
    c = cases[name]
    compare(name, c["P"], c["V"], c["F"], c["g"], c["r64"], (c["E32_dP"], c["E32_dV"]))
    compare(name + " d >= 1e-2", c["P"], c["V"], c["F"], c["g_sharp"], c["s64"], (c["E32_dP_sharp"], c["E32_dV_sharp"]))


@pytest.mark.parametrize("N", [1, 255, 257, 511, 513])
def test_shapes_points(cases, N):
    """the first N points of ico2: one chunk, a second chunk of one point, three chunks.  N = 1: the largest error of ONE point
    of the restatement is no measure of float32 arithmetic (here 1.8e-8, by the luck of its roundings), so its E32 is taken
    over the first 255 points, which are of its kind (surface samples with sigma 0.08 and uniform ones)"""
    c = cases["ico2"]
    if N >= 255:
        compare("ico2 N=%d" % N, c["P"][:N], c["V"], c["F"], c["g"][:N])
    else:
        E = gref._e32(c["P"][:255], c["V"], c["F"], c["g"][:255])[1:]
        compare("ico2 N=%d" % N, c["P"][:N], c["V"], c["F"], c["g"][:N], gref.grads(c["P"][:N], c["V"], c["F"], c["g"][:N]), E)


@pytest.mark.parametrize("slots", [255, 257])
def test_shapes_vertices(cases, slots):
    """ico2's 162 vertices scattered over 255 / 257 slots, the last slot used; the unreferenced slots get exactly 0"""
    c = cases["ico2"]
    perm = np.random.RandomState(slots).permutation(slots - 1)[:161]
    where = np.concatenate([perm, [slots - 1]])                     # where the mesh's vertices go: 161 random slots and the last
    V = np.full((slots, 3), 9.0) + np.arange(slots)[:, None]        # far away, unused
    V[where] = c["V"]
    F = where[c["F"]]
    r64, eP, eV = gref._e32(c["P"], V, F, c["g"])
    assert np.abs(r64["dV"][where] - c["r64"]["dV"]).max() <= 1e-12
    dP, dV = compare("ico2 in %d slots" % slots, c["P"], V, F, c["g"], r64, (eP, eV))
    unused = np.setdiff1d(np.arange(slots), where)
    assert (dV[unused] == 0).all() and np.abs(dV[slots - 1]).max() > 0
    _, dP0, dV0 = gpu_grads(c["P"], c["V"], c["F"], c["g"])         # the same sums at other thread positions
    assert np.array_equal(dV[where], dV0) and np.array_equal(dP, dP0)


def test_chunk_cap(cases):
    """N = 16 385 points about the 12-face box: 65 record tiles, S = 64 chunks"""
    c = cases["box12"]
    P = f32(np.random.RandomState(8).rand(16385, 3) * 1.6 + np.array([-0.8, -0.7, 1.5]))
    tie = gref.ties(P, c["V"], c["F"], 8 * gref.e32_dist(P, c["V"], c["F"]))
    print("N=16385: %d ties" % tie.sum())
    assert tie.sum() <= gref.TIE_CAP * len(P)
    g = np.where(tie, 0.0, f32(np.random.RandomState(9).uniform(0.5, 1.5, len(P))))
    compare("box12 N=16385", P, c["V"], c["F"], g)


def test_batched(cases):
    """B = 3 on ico2, a different mesh in every frame (shifted, scaled) and different points: every frame against its own"""
    from chore_amd.preprocess import mesh_distance
    c = cases["ico2"]
    Vs = [c["V"], f32(c["V"] + np.array([0.3, 0.0, 0.0])), f32((c["V"] - c["V"].mean(0)) * 1.3 + c["V"].mean(0))]
    Ps = [c["P"], c["P"][::-1].copy(), f32(c["P"] + np.array([0.01, -0.02, 0.005]))]
    gs, refs = [], []
    for P, V in zip(Ps, Vs):
        tie = gref.ties(P, V, c["F"], 8 * gref.e32_dist(P, V, c["F"]))
        assert tie.sum() <= gref.TIE_CAP * len(P)
        gs.append(np.where(tie, 0.0, np.abs(c["g"]) + (c["g"] == 0)))
        refs.append(gref._e32(P, V, c["F"], gs[-1]))
    p, v = dev(np.stack(Ps), np.float32).requires_grad_(True), dev(np.stack(Vs), np.float32).requires_grad_(True)
    d = mesh_distance(p, v, dev(c["F"], np.int32), "dist")
    assert tuple(d.shape) == (3, 600) and d.requires_grad
    d.backward(dev(np.stack(gs), np.float32))
    dP, dV = p.grad.cpu().numpy(), v.grad.cpu().numpy()
    assert dP.shape == (3, 600, 3) and dV.shape == (3, 162, 3)
    for b, (r64, eP, eV) in enumerate(refs):
        errP, errV = np.abs(dP[b] - r64["dP"]).max(), np.abs(dV[b] - r64["dV"]).max()
        print("B=3 frame %d: dpoints %.3e (E32 %.3e)  dverts %.3e (E32 %.3e)" % (b, errP, eP, errV, eV))
        assert 0 < eP < 1e-2 and 0 < eV < 1e-2 and errP <= 8 * eP and errV <= 8 * eV
        one = gpu_grads(Ps[b], Vs[b], c["F"], gs[b])                # B = 1 has the same number of chunks here: the same bits
        assert np.array_equal(one[1], dP[b]) and np.array_equal(one[2], dV[b])


@pytest.mark.parametrize("name", ["ico2", "box12"])
def test_signed_gradient_is_the_distance_gradient_with_the_sign(cases, name):
    """2: signed (sign_mode='inside'): its gradient is where(inside, -1, +1) times that of dist, bit for bit"""
    from chore_amd.preprocess import mesh_distance
    c = cases[name]
    inside = mesh_distance(dev(c["P"], np.float32), dev(c["V"], np.float32), dev(c["F"], np.int32), "inside").cpu().numpy()
    assert 0 < inside.sum() < len(inside)
    g = c["g"].astype(np.float32)
    sd, sP, sV = gpu_grads(c["P"], c["V"], c["F"], g, want="signed")
    d, dP, dV = gpu_grads(c["P"], c["V"], c["F"], g)
    assert np.array_equal(sd.view(np.uint32), np.where(inside, -d, d).view(np.uint32))
    on = (d > 0) & (g != 0)
    assert np.array_equal(sP[on].view(np.uint32), np.where(inside[:, None], -dP, dP)[on].view(np.uint32))
    assert np.array_equal(sP, np.where(inside[:, None], -dP, dP))
    _, _, fV = gpu_grads(c["P"], c["V"], c["F"], np.where(inside, -g, g))      # the vertex sums: those of dist under the signed g
    assert np.array_equal(sV.view(np.uint32), fV.view(np.uint32))
    allin = gpu_grads(c["P"][inside], c["V"], c["F"], g[inside], want="signed")[2]
    assert np.array_equal(allin, -gpu_grads(c["P"][inside], c["V"], c["F"], g[inside])[2])


def test_hot_vertex(cases):
    """3: 1 000 points in the octant beyond one corner of the 12-face box: every contribution lands on that corner, the other
    seven vertices get exactly 0, the sum is within 8 x its own E32"""
    c = cases["box12"]
    corner = c["V"].max(0)
    k = int(np.nonzero((c["V"] == corner).all(1))[0][0])
    P = f32(corner + 0.01 + 0.5 * np.random.RandomState(6).rand(1000, 3))
    g = f32(np.random.RandomState(7).uniform(0.5, 1.5, 1000))
    assert not gref.ties(P, c["V"], c["F"], 8 * gref.e32_dist(P, c["V"], c["F"])).any()
    r64, eP, eV = gref._e32(P, c["V"], c["F"], g)
    assert (np.delete(r64["dV"], k, 0) == 0).all() and np.abs(r64["dV"][k] + r64["dP"].sum(0)).max() <= 1e-9
    dP, dV = compare("hot vertex", P, c["V"], c["F"], g, r64, (eP, eV))
    assert (np.delete(dV, k, 0) == 0).all()
    assert np.abs(dV[k]).min() > 100


def test_null_rule_and_degenerate_input(cases):
    """4: dpoints-only and dverts-only calls have the bits of the both-call; an unreferenced vertex is exactly 0; 200 appended
    zero-area faces change no bit; points ON vertices (dist == 0) give zero rows and finite everything"""
    c = cases["ico2"]
    V = np.concatenate([c["V"], [[5.0, 5.0, 5.0]]])                    # vertex 162: referenced by no face
    both = gpu_grads(c["P"], V, c["F"], c["g"])
    onlyp = gpu_grads(c["P"], V, c["F"], c["g"], dv=False)
    onlyv = gpu_grads(c["P"], V, c["F"], c["g"], dp=False)
    assert onlyp[2] is None and onlyv[1] is None
    assert np.array_equal(onlyp[1].view(np.uint32), both[1].view(np.uint32))
    assert np.array_equal(onlyv[2].view(np.uint32), both[2].view(np.uint32))
    assert (both[2][162] == 0).all() and np.abs(both[2][:162]).max() > 0
    # zero-area faces that lie ON the mesh (a chord between two vertices of the sphere would be nearer to inside points than the
    # surface is): corner 0 of a face three times, and corners (0, 0, 2) of a face -- the segment whose distance that face
    # itself forms with the same arithmetic (its edge ac), so the face, with the smaller index, keeps every tie
    rs = np.random.RandomState(4)
    r = rs.randint(0, len(c["F"]), 200)
    i, j = c["F"][r, 0], c["F"][r, 2]
    deg = np.concatenate([np.stack([i, i, i], 1)[:100], np.stack([i, i, j], 1)[100:]])[rs.permutation(200)]
    more = gpu_grads(c["P"], V, np.concatenate([c["F"], deg]), c["g"])
    for a, b in zip(both, more):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # degenerate faces alone (segments and a point): finite, and the weights sum to 1 -- the vertex sums add up to -sum dpoints
    alone = gpu_grads(c["P"][:100], V, deg, np.ones(100))
    assert all(np.isfinite(a).all() for a in alone)
    assert np.abs(alone[2].astype(np.float64).sum(0) + alone[1].astype(np.float64).sum(0)).max() <= 1e-4
    # points exactly on vertices: dist == 0, zero rows
    Pon = f32(np.concatenate([c["V"][:40], c["P"][:60]]))
    d, dP, dV = gpu_grads(Pon, V, c["F"], np.ones(100))
    assert (d[:40] == 0).all() and (dP[:40] == 0).all() and np.isfinite(dP).all() and np.isfinite(dV).all()
    _, _, dV60 = gpu_grads(Pon[40:], V, c["F"], np.ones(60))
    assert np.array_equal(dV, dV60)                                   # the points on vertices contribute exactly 0


def test_reproducible_and_capturable(cases):
    """5: two calls and a graph replay of forward + backward give the same bits"""
    from chore_amd.preprocess import mesh_distance
    c = cases["body"]
    p, v = dev(c["P"], np.float32).requires_grad_(True), dev(c["V"], np.float32).requires_grad_(True)
    f, g = dev(c["F"], np.int32), dev(c["g"], np.float32)

    def call():
        d = mesh_distance(p, v, f, "signed")
        dp, dv = torch.autograd.grad(d, (p, v), g)
        return d.detach(), dp, dv
    a, b = call(), call()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[1].abs().max() > 0 and a[2].abs().max() > 0
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cc = call()
    for _ in range(2):
        for t in cc:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(a, cc):
            assert torch.equal(x, y)


def test_forward_bits_and_no_grad(cases):
    """6: with requires_grad inputs dist, signed and the other outputs have the bits of the detached call; the other outputs
    carry no graph; under no_grad no graph is built"""
    from chore_amd.preprocess import mesh_distance
    c = cases["ico2"]
    names = ("dist", "face_idx", "closest", "vert_idx", "winding", "inside", "signed")
    p, v, f = dev(c["P"], np.float32), dev(c["V"], np.float32), dev(c["F"], np.int32)
    plain = mesh_distance(p, v, f, names)
    assert not any(t.requires_grad for t in plain)
    pg, vg = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    out = mesh_distance(pg, vg, f, names)
    for k, a, b in zip(names, plain, out):
        assert torch.equal(a, b) and a.dtype == b.dtype, k
        assert b.requires_grad == (k in ("dist", "signed")), k
    only = mesh_distance(pg, v, f, "dist")                       # one input that requires grad is enough
    assert only.requires_grad and torch.equal(only, plain[0])
    frac = mesh_distance(pg, vg, f, ("signed", "closest"), sign_mode="winding")
    assert not frac[0].requires_grad and not frac[1].requires_grad
    assert torch.equal(frac[0], mesh_distance(p, v, f, "signed", sign_mode="winding"))
    with torch.no_grad():
        ng = mesh_distance(pg, vg, f, ("dist", "signed"))
    assert not ng[0].requires_grad and ng[0].grad_fn is None and torch.equal(ng[0], plain[0]) and torch.equal(ng[1], plain[6])
    one = mesh_distance(pg[:7], vg, f, "dist")                   # unbatched in, unbatched gradients out
    one.sum().backward()
    assert tuple(pg.grad.shape) == (600, 3) and tuple(vg.grad.shape) == (162, 3) and (pg.grad[7:] == 0).all()
    h = pg.detach().double().requires_grad_(True)                # another dtype: the gradient comes back in it
    mesh_distance(h, v, f, "dist").sum().backward()
    assert h.grad.dtype == torch.float64 and torch.equal(h.grad[:7].float(), pg.grad[:7])


def test_refusals():
    """7: CPU tensors raise, unsupported shapes raise ValueError, with and without a gradient asked for"""
    from chore_amd import _lib
    from chore_amd.preprocess import mesh_distance
    p, v, f = torch.zeros(4, 3), torch.eye(3), torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError):
        mesh_distance(p.requires_grad_(True), v.cuda(), f.cuda())
    with pytest.raises(RuntimeError):
        mesh_distance(p.detach().cuda(), v.requires_grad_(True), f.cuda())
    for grad in (False, True):
        with pytest.raises(ValueError):
            mesh_distance(torch.zeros(0, 3).cuda().requires_grad_(grad), v.detach().cuda(), f.cuda())
        with pytest.raises(ValueError):
            mesh_distance(torch.zeros(4, 2).cuda().requires_grad_(grad), v.detach().cuda(), f.cuda())
    assert _lib.lib.chore_mesh_dist_bwd_workspace_bytes(1, 0, 3, 1) == 0
    assert _lib.lib.chore_mesh_dist_bwd_workspace_bytes(1, 1 << 27, 3, 1) == 0
    assert _lib.lib.chore_mesh_dist_bwd_workspace_bytes(2, 600, 162, 320) > 0
