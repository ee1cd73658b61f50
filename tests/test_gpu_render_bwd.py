"""GPU: the backward of the HIP colour / depth rasteriser (chore_render_bwd) and the autograd path of
chore_amd.render.Renderer against the numpy restatement (tests/render_bwd_ref.py), the silhouette backward
(chore_silhouette_bwd), the reference's known answers and torch's own autograd."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import render_bwd_cases as cases
import render_bwd_ref
from render_bwd_cases import BG, DEPTH_TRI, EPS, EYE, FAR, NEAR, RGB_CASES, TEX_EPS

pytestmark = pytest.mark.gpu


def dev(a):
    if a is None or torch.is_tensor(a):
        return a
    return torch.as_tensor(np.asarray(a, np.float32)).cuda().contiguous()


def hip_forward(tri, tex, light, size, ssaa, bg=BG, eps=TEX_EPS):
    from chore_amd.render import rasterize_rgbad
    with torch.no_grad():
        return rasterize_rgbad(dev(tri), dev(tex), dev(light), size, ssaa == 2, NEAR, FAR, eps, bg, return_index=True)


def hip_backward(tri, tex, light, fim, size, ssaa, g_rgb, g_depth, g_alpha, eps=EPS, tex_eps=TEX_EPS, bg=BG, textures=True,
                 with_light=True):
    """one chore_render_bwd call on device tensors (tri, tex, light, the gradients: fp32; fim int32) -> dict of tensors"""
    from chore_amd import _lib
    B, Fn, ts = tri.shape[0], tri.shape[1], tex.shape[2]
    h = _lib.handle(0)
    nbytes = _lib.lib.chore_render_bwd_workspace_bytes(B, Fn, ts, size, ssaa)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = {"tri": torch.full_like(tri, 7.0)}
    if textures:
        out["textures"] = torch.full_like(tex, 7.0)
    if with_light and light is not None:
        out["light"] = torch.full_like(light, 7.0)
    ptr = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
    _lib.check(_lib.lib.chore_render_bwd(h, tri.data_ptr(), tex.data_ptr(), ptr(light), fim.data_ptr(), B, Fn, ts, size, ssaa,
                                         NEAR, FAR, tex_eps, eps, (ctypes.c_float * 3)(*bg), ptr(g_rgb), ptr(g_depth),
                                         ptr(g_alpha), out["tri"].data_ptr(), ptr(out.get("textures")), ptr(out.get("light")),
                                         ws.data_ptr(), torch.cuda.current_stream().cuda_stream), h, "chore_render_bwd")
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """the case, its forward on the kernels, and the restatement in float64 and float32 on the kernel's own winners"""
    c = {"A": lambda: cases.random_case(1, 2, 64, 1), "B": lambda: cases.random_case(1, 3, 24, 2), "tie": cases.tie_case,
         "large": cases.large_face_case, "multibin": cases.multi_bin_case}[name]()
    fwd = hip_forward(c["tri"], c["tex"], c["light"], c["size"], c["ssaa"])
    fim = fwd["face_index"].cpu().numpy()
    ref = {dt: render_bwd_ref.render_bwd(c["tri"], c["tex"], c["light"], fim, c["ssaa"], c["g_rgb"], c["g_depth"], c["g_alpha"],
                                         NEAR, FAR, TEX_EPS, EPS, BG, dt) for dt in (np.float64, np.float32)}
    t = {k: dev(c[k]) for k in ("tri", "tex", "light", "g_rgb", "g_depth", "g_alpha")}
    t["fim"] = fwd["face_index"]
    return c, t, fim, ref


def call(t, c, rgb=True, depth=True, alpha=True, **kw):
    return hip_backward(t["tri"], t["tex"], t["light"], t["fim"], c["size"], c["ssaa"], t["g_rgb"] if rgb else None,
                        t["g_depth"] if depth else None, t["g_alpha"] if alpha else None, **kw)


@pytest.mark.parametrize("name", ["A", "B", "tie", "large", "multibin"])
def test_kernel_against_restatement(name):
    """6: chore_render_bwd on the kernel's own sample_face_index against the float64 restatement; all three upstream gradients
    standard normal, a non-zero background, the light in [0.3, 1].  The pixel-map term is called alone (no depth gradient),
    the depth term alone, and the full call is their sum bit for bit.  Bound: 1e-4 of the largest entry of each output
    (tests/test_gpu_silhouette.py's).  A face is left out of the pixel-map comparison only where the restatement in float32
    itself misses that bound against float64 (a discrete decision of the walk taken differently), at most 2 % of the faces
    with a gradient: seed 1 leaves out one face of 75 in A and none in the other cases (chosen on the CPU, where the float32
    restatement on the silhouette restatement's winners shows the same)."""
    c, t, fim, ref = case(name)
    r64, r32 = ref[np.float64], ref[np.float32]
    B, Fn = c["tri"].shape[:2]
    assert 0.3 < (fim >= 0).mean() < 0.97
    if name == "tie":
        assert (fim == 1).sum() > 50 and not (fim == 3).any()
    if name == "large":
        assert (fim == 0).mean() > 0.5
    pm = call(t, c, depth=False)
    dp = call(t, c, rgb=False, alpha=False)
    full = call(t, c)
    assert torch.equal(full["tri"], pm["tri"] + dp["tri"])
    assert torch.equal(full["textures"], pm["textures"]) and torch.equal(full["light"], pm["light"])
    assert not dp["textures"].any() and not dp["light"].any()

    want = r64["pixel_map"]
    bound = 1e-4 * np.abs(want).max()
    out = cases.leave_out(r32["pixel_map"], want, bound)
    nonzero = np.abs(want).reshape(B, Fn, -1).max(-1) > 0
    err = np.abs(pm["tri"].cpu().numpy().astype(np.float64) - want).reshape(B, Fn, -1).max(-1)
    print("%s pixel map: largest %.4g bound %.3g error %.3g (kept faces), faces with a gradient %d, left out %d"
          % (name, np.abs(want).max(), bound, err[~out].max(), nonzero.sum(), out.sum()))
    assert nonzero.sum() >= 5 and out.sum() <= 0.02 * nonzero.sum()
    assert np.all(want[..., 2] == 0) and not pm["tri"][..., 2].any()
    assert err[~out].max() <= bound

    for key, got in (("depth", dp["tri"]), ("textures", pm["textures"]), ("light", pm["light"])):
        want = r64[key]
        bound = 1e-4 * np.abs(want).max()
        e32 = np.abs(r32[key].astype(np.float64) - want).max()
        e = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print("%s %s: largest %.4g bound %.3g error %.3g (float32 restatement %.3g)" % (name, key, np.abs(want).max(), bound, e, e32))
        assert got.shape == want.shape and np.abs(want).max() > 0.1
        assert e <= bound, (name, key, e, bound)


def test_silhouette_consistency():
    """7: with grad_alpha alone at ssaa 1 (rows reversed: the silhouette entry point does not flip) the result is
    chore_silhouette_bwd's bit for bit"""
    from chore_amd import _lib
    c, t, fim, _ = case("A")
    B, Fn, S = c["tri"].shape[0], c["tri"].shape[1], c["size"]
    got = hip_backward(t["tri"], t["tex"], t["light"], t["fim"], S, 1, None, None, t["g_alpha"], eps=1e-4)
    h = _lib.handle(0)
    alpha = (t["fim"] >= 0).float().contiguous()
    ga = t["g_alpha"].flip(1).contiguous()
    want = torch.full_like(t["tri"], 7.0)
    _lib.check(_lib.lib.chore_silhouette_bwd(h, t["tri"].data_ptr(), t["fim"].data_ptr(), alpha.data_ptr(), ga.data_ptr(), B, Fn,
                                             S, 1e-4, want.data_ptr(), torch.cuda.current_stream().cuda_stream), h, "sil_bwd")
    assert want.abs().max() > 1
    assert torch.equal(got["tri"], want)
    assert not got["textures"].any() and not got["light"].any()


def test_anti_aliasing_consistency():
    """8: the gradients of an ssaa 2 call at size s equal those of an ssaa 1 call at size 2 s followed by avg_pool2d(2), for
    the same upstream gradient, to 1e-6 of the largest entry (they differ in the order of four-term sums only)"""
    c, t, fim, _ = case("B")
    s = c["size"]
    two = call(t, c)
    one_fwd = hip_forward(c["tri"], c["tex"], c["light"], 2 * s, 1)
    assert torch.equal(one_fwd["face_index"], t["fim"])
    ups = []
    for g in (t["g_rgb"], t["g_depth"][:, None], t["g_alpha"][:, None]):
        x = torch.zeros(g.shape[0], g.shape[1], 2 * s, 2 * s, device="cuda", requires_grad=True)
        F.avg_pool2d(x, 2).backward(g)
        ups.append(x.grad.contiguous())
    one = hip_backward(t["tri"], t["tex"], t["light"], t["fim"], 2 * s, 1, ups[0], ups[1][:, 0].contiguous(),
                       ups[2][:, 0].contiguous())
    for k in ("tri", "textures", "light"):
        big = one[k].abs().max().item()
        e = (one[k] - two[k]).abs().max().item()
        print("%s: largest %.4g difference %.3g" % (k, big, e))
        assert big > 0.1 and e <= 1e-6 * big, k


def test_null_is_zero_reproducible_and_capturable():
    """10: a NULL upstream pointer and a zero tensor give equal bits; two calls are bit-equal; forward + backward captured
    into one graph on one stream replay to the eager bits"""
    from chore_amd.render import rasterize_rgbad
    c, t, fim, _ = case("B")
    zero3, zero1 = torch.zeros_like(t["g_rgb"]), torch.zeros_like(t["g_depth"])
    for rgb, depth, alpha in ((False, True, True), (True, False, True), (True, True, False), (False, True, False),
                              (False, False, True), (False, False, False)):
        a = call(t, c, rgb, depth, alpha)
        b = hip_backward(t["tri"], t["tex"], t["light"], t["fim"], c["size"], c["ssaa"], t["g_rgb"] if rgb else zero3,
                         t["g_depth"] if depth else zero1, t["g_alpha"] if alpha else zero1)
        for k in a:
            assert torch.equal(a[k], b[k]), (rgb, depth, alpha, k)
        if not (rgb or depth or alpha):
            assert not any(v.any() for v in a.values())
    eager, again = call(t, c), call(t, c)
    for k in eager:
        assert torch.equal(eager[k], again[k]), k
    few = call(t, c, textures=False, with_light=False)           # the nullable outputs
    assert set(few) == {"tri"} and torch.equal(few["tri"], eager["tri"])

    def both():
        out = rasterize_rgbad(t["tri"], t["tex"], t["light"], c["size"], c["ssaa"] == 2, NEAR, FAR, TEX_EPS, BG, return_index=True)
        return out, hip_backward(t["tri"], t["tex"], t["light"], out["face_index"], c["size"], c["ssaa"], t["g_rgb"],
                                 t["g_depth"], t["g_alpha"])
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side), torch.no_grad():
        both()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side), torch.no_grad():
        fwd, bwd = both()
    for _ in range(2):
        for v in list(fwd.values()) + list(bwd.values()):
            v.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(fwd["face_index"], t["fim"])
        for k in eager:
            assert torch.equal(eager[k], bwd[k]), k


def small_mesh():
    from meshes import icosphere
    v, f = icosphere(1, 0.5, (0.1, -0.1, 2.2))
    return torch.from_numpy(v.astype(np.float32))[None].cuda(), torch.from_numpy(f.astype(np.int64))[None].cuda()


def small_renderer(size=32):
    from chore_amd.utils.render_utils import setup_renderer
    return setup_renderer(image_size=size)


def test_gradients_exist():
    """3: render_depth, render_rgb and render on inputs that require grad give outputs with a grad_fn and finite non-zero
    gradients"""
    r = small_renderer()
    assert r.camera_mode == "projection"
    v0, f = small_mesh()
    tex0 = torch.rand(1, f.shape[1], 2, 2, 2, 3, device="cuda")

    def check(run, wants_tex):
        v, tex = v0.clone().requires_grad_(), tex0.clone().requires_grad_()
        outs = run(v, tex)
        outs = outs if isinstance(outs, tuple) else (outs,)
        assert all(o.grad_fn is not None for o in outs)
        sum((o * torch.randn_like(o)).sum() for o in outs).backward()
        assert torch.isfinite(v.grad).all() and v.grad.abs().max() > 0
        if wants_tex:
            assert torch.isfinite(tex.grad).all() and tex.grad.abs().max() > 0
        else:
            assert tex.grad is None
    check(lambda v, tex: r.render_depth(v, f), False)
    check(lambda v, tex: r(v, f, mode="depth"), False)
    check(lambda v, tex: r.render_rgb(v, f, tex), True)
    check(lambda v, tex: r.render(v, f, tex), True)
    check(lambda v, tex: r(v, f, tex), True)
    with torch.no_grad():
        assert r.render_depth(v0.clone().requires_grad_(), f).grad_fn is None


def test_forward_unchanged():
    """4: with inputs that require grad the outputs are torch.equal to those with detached inputs"""
    r = small_renderer()
    v, f = small_mesh()
    tex = torch.rand(1, f.shape[1], 3, 3, 3, 3, device="cuda")
    plain = r.render(v, f, tex)
    tracked = r.render(v.clone().requires_grad_(), f, tex.clone().requires_grad_())
    for a, b in zip(plain, tracked):
        assert a.grad_fn is None and b.grad_fn is not None and torch.equal(a, b)
    assert torch.equal(r.render_depth(v, f), r.render_depth(v.clone().requires_grad_(), f))
    assert torch.equal(r.render_rgb(v, f, tex), r.render_rgb(v, f, tex.clone().requires_grad_()))
    assert torch.equal(r.render_silhouettes(v, f), r.render_silhouettes(v.clone().requires_grad_(), f))


def kernels_tri(v, fill=True):
    """look_at (identity rotation, no perspective: v - eye) or nothing, vertices_to_faces with both windings"""
    from chore_amd.render import vertices_to_faces
    f = torch.tensor([[[0, 1, 2]]], device="cuda")
    return vertices_to_faces(v, torch.cat((f, f.flip(-1)), 1) if fill else f)


@pytest.mark.parametrize("verts,pix,minus_one,ref", RGB_CASES)
def test_reference_rgb_known_answers(verts, pix, minus_one, ref):
    """5: external/neural_renderer/tests/test_rasterize.py:84-156 through look_at + vertices_to_faces + rasterize_rgbad on the
    kernels, size 64 without anti-aliasing, at that test's own rtol"""
    from chore_amd.render import look_at, rasterize_rgbad
    v = torch.tensor([verts], device="cuda").requires_grad_()
    tri = kernels_tri(look_at(v, EYE.tolist()))
    tex = torch.ones(1, 2, 4, 4, 4, 3, device="cuda")
    light = torch.ones(1, 2, 3, device="cuda")
    out = rasterize_rgbad(tri, tex, light, 64, False, NEAR, FAR, 1e-3, (0, 0, 0))
    image = out["rgb"].mean(1)
    loss = torch.sum(torch.abs(image[:, pix[0], pix[1]] - (1 if minus_one else 0)))
    loss.backward()
    np.testing.assert_allclose(v.grad[0].cpu().numpy(), np.array(ref, np.float32), rtol=1e-2, atol=1e-6)


def test_reference_depth_finite_differences():
    """5: external/neural_renderer/tests/test_rasterize_depth.py:57-90 on the kernels: the gradient of (d - 1)^2 at pixel
    (15, 20) against forward differences of step 1e-3 of the kernels' own forward, atol 1e-3"""
    from chore_amd.render import rasterize_rgbad
    tex = torch.ones(1, 2, 2, 2, 2, 3, device="cuda")

    def loss_of(v):
        return (rasterize_rgbad(kernels_tri(v), tex, None, 64, False, NEAR, FAR, 1e-3)["depth"][0, 15, 20] - 1) ** 2
    v = torch.tensor([DEPTH_TRI], device="cuda").requires_grad_()
    loss = loss_of(v)
    loss.backward()
    fd = torch.zeros(3, 3)
    for i in range(3):
        for j in range(3):
            v2 = v.detach().clone()
            v2[0, i, j] += 1e-3
            fd[i, j] = ((loss_of(v2) - loss.detach()) / 1e-3).item()
    print(v.grad[0].cpu(), fd, (v.grad[0].cpu() - fd).abs().max())
    assert v.grad.abs().max() > 0.1
    assert torch.allclose(v.grad[0].cpu(), fd, rtol=0, atol=1e-3)


def test_autograd_chain():
    """9: Renderer.render with the directional light on: vertices.grad equals the C call's grad_tri and grad_light pushed by
    hand through torch's transform, vertices_to_faces and face_light; textures.grad equals the C call's grad_textures folded
    over fill_back's two copies"""
    from chore_amd.render import face_light, vertices_to_faces
    r = small_renderer()
    assert r.fill_back and r.light_intensity_directional > 0 and r.anti_aliasing
    v0, f = small_mesh()
    Fn = f.shape[1]
    tex0 = torch.rand(1, Fn, 2, 2, 2, 3, device="cuda")
    v, tex = v0.clone().requires_grad_(), tex0.clone().requires_grad_()
    outs = r.render(v, f, tex)
    ups = [torch.randn_like(o) for o in outs]
    torch.autograd.backward(outs, ups)
    # by hand
    f2 = torch.cat((f, f.flip(-1)), 1)
    vh = v0.clone().requires_grad_()
    tri = vertices_to_faces(r.transform(vh), f2)
    light = face_light(vertices_to_faces(vh, f2), r.light_intensity_ambient, r.light_intensity_directional,
                       r.light_color_ambient, r.light_color_directional, r.light_direction)
    tex2 = torch.cat((tex0, tex0.permute((0, 1, 4, 3, 2, 5))), 1).contiguous()
    fwd = hip_forward(tri.detach(), tex2, light.detach(), r.image_size, 2, tuple(r.background_color), r.rasterizer_eps)
    for a, b in zip(outs, (fwd["rgb"], fwd["depth"], fwd["alpha"])):
        assert torch.equal(a, b)
    got = hip_backward(tri.detach().contiguous(), tex2, light.detach().contiguous(), fwd["face_index"], r.image_size, 2,
                       ups[0].contiguous(), ups[1].contiguous(), ups[2].contiguous(), eps=r.rasterizer_eps,
                       tex_eps=r.rasterizer_eps, bg=tuple(float(x) for x in r.background_color))
    torch.autograd.backward([tri, light], [got["tri"], got["light"]])
    assert got["light"].abs().max() > 0 and vh.grad.abs().max() > 0
    e = (v.grad - vh.grad).abs().max().item()
    print("vertices.grad: largest %.4g, difference to the hand-made chain %.3g" % (vh.grad.abs().max().item(), e))
    assert e <= 1e-6 * vh.grad.abs().max().item()            # the same operations; torch's scatter order is its own
    folded = got["textures"][:, :Fn] + got["textures"][:, Fn:].permute((0, 1, 4, 3, 2, 5))
    assert folded.abs().max() > 0
    assert torch.equal(tex.grad, folded)


def test_look_on_the_device():
    """11: chore_amd.render.look on device tensors against the fixture the reference's look.py wrote (tests/golden/look.npz);
    `Renderer(camera_mode='look')` itself still refuses (tests/test_render_host.py pins that)"""
    from chore_amd.render import look
    from conftest import golden
    g = golden("look.npz")
    v = torch.from_numpy(g["vertices"]).cuda().requires_grad_()
    for name in ("default_up", "oblique", "batched"):
        eye, direction, up = (torch.from_numpy(g["%s_%s" % (k, name)]).cuda() for k in ("eye", "direction", "up"))
        got = look(v, eye, direction, up)
        assert got.is_cuda and np.abs(got.detach().cpu().numpy() - g["out_" + name]).max() <= 4 * float(g["bound_" + name])
    got.sum().backward()
    assert torch.isfinite(v.grad).all() and v.grad.abs().max() > 0
