"""Renderer.shading_vectors on the GPU against tests/shading_ref.py, on rasterize's own output: two views taken as [1, 0], a
40 x 24 frame (no multiple of 16), L = 1 and 4, ray tensors and analytic rays; the forward bit for bit, view = -ray_d, a window at
unaligned origins equal to the crop of the frame, gradients per element within  |g - g64| <= 1e-5 max|g64| + 8 eps32 sum|terms|
(util.summation_bound) with one output at a time in the loss, empty and invalid slots, the argument checks down to the C ABI, and
the module path rasterize -> interpolate(vertex_normals) -> shading_vectors -> texture(cube) -> composite -> backward."""
import functools

import numpy as np
import pytest
import torch

import shading_ref as sref
from util import patched_C, scenes, summation_bound

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, BIDX = 40, 24, [1, 0]
MODES = ("tensors", "analytic")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene():
    return scenes.tet_lattice(W, H, 3, seed=scenes.SEED_BASE + 91, num_cams=2)


def _renderer(mode):
    ts = _scene().to("cuda")
    return ts, dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda", analytic_rays=mode == "analytic")


def _rays(r, mode):
    """The rays of the selected views over the full frame, numpy (B,H,W,3): the renderer's own tensors, or the oracle's
    restatement of the computed ray."""
    if mode == "analytic":
        from oracle import cpu as orc
        cam = _np(r.ray_cam)[BIDX]
        return orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), W, H)
    pm = torch.zeros((len(BIDX), 2), dtype=torch.int32, device="cuda")
    ro, rd = r.select_rays(BIDX, pm, W, H)
    return _np(ro).astype(f32), _np(rd).astype(f32)


@functools.lru_cache(maxsize=None)
def _case(mode, L):
    """rasterize's output for the lattice and a normal image of mixed lengths, numpy, with the rays: computed once per (mode, L)."""
    ts, r = _renderer(mode)
    layers, cnt, bary, t = r.rasterize(BIDX, ts.verts, ts.faces, L)
    vn = r.vertex_normals(ts.verts, ts.faces) * (0.25 + 3.0 * torch.rand((ts.verts.shape[0], 1), generator=torch.Generator().manual_seed(5)).cuda())
    nimg = r.interpolate(layers, bary, vn, ts.faces)
    ro, rd = _rays(r, mode)
    c = dict(layers=_np(layers), t=_np(t), normals=_np(nimg), ro=ro, rd=rd)
    assert (c["layers"] >= 0).sum() > 200 and (c["layers"] < 0).any() and (c["t"][c["layers"] < 0] == -1).all()
    return c


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g = _np(g)
        assert g.shape == w.shape and g.dtype == np.float32, (what, k)
        assert np.array_equal(_bits(g), _bits(w)), (what, k, int((_bits(g) != _bits(w)).sum()))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [1, 4])
def test_forward_bit_equal_to_the_restatement(mode, L):
    c = _case(mode, L)
    _, r = _renderer(mode)
    got4 = r.shading_vectors(BIDX, _cu(c["layers"]), _cu(c["t"]), _cu(c["normals"]))
    got2 = r.shading_vectors(BIDX, _cu(c["layers"]), _cu(c["t"]))
    torch.cuda.synchronize()
    _same(got4, sref.forward32(c["layers"], c["t"], c["normals"], c["ro"], c["rd"]), (mode, L, "with normals"))
    _same(got2, sref.forward32(c["layers"], c["t"], None, c["ro"], c["rd"]), (mode, L, "without"))
    live = c["layers"] >= 0
    view = _np(got4[1])
    want = np.broadcast_to(-c["rd"][:, :, :, None, :], view.shape)
    assert np.array_equal(_bits(view[live]), _bits(np.ascontiguousarray(want[live])))
    assert not view[~live].any() and not _np(got4[0])[~live].any()
    length = lambda a: np.linalg.norm(a[live].astype(np.float64), axis=-1)
    assert np.abs(length(_np(got4[3])) - length(view)).max() <= 1e-6       # a mirror image: as unit as the rays are
    assert type(r).shading_vectors is dm2.Renderer.shading_vectors


@pytest.mark.parametrize("mode", MODES)
def test_window_equals_the_crop_of_the_frame(mode):
    L = 4
    c = _case(mode, L)
    _, r = _renderer(mode)
    full = [_np(x) for x in r.shading_vectors(BIDX, _cu(c["layers"]), _cu(c["t"]), _cu(c["normals"]))]
    pm = np.array([[3, 5], [17, 2]], np.int32)                             # unaligned, another origin per view
    pw, ph = 19, 13
    cut = lambda a: np.stack([a[b, pm[b, 1]:pm[b, 1] + ph, pm[b, 0]:pm[b, 0] + pw] for b in range(2)])
    got = r.shading_vectors(BIDX, _cu(cut(c["layers"])), _cu(cut(c["t"])), _cu(cut(c["normals"])), patch_min=_cu(pm))
    torch.cuda.synchronize()
    _same(got, [cut(a) for a in full], (mode, "window"))
    _same(got, sref.forward32(cut(c["layers"]), cut(c["t"]), cut(c["normals"]), cut(c["ro"]), cut(c["rd"])), (mode, "window, restated"))
    assert (cut(c["layers"]) >= 0).sum() > 50
    # the gradient of a window is the crop's as well
    tl, nl = _cu(cut(c["t"])).requires_grad_(True), _cu(cut(c["normals"])).requires_grad_(True)
    outs = r.shading_vectors(BIDX, _cu(cut(c["layers"])), tl, nl, patch_min=_cu(pm))
    gs = [np.random.default_rng(40 + k).standard_normal(outs[0].shape).astype(f32) for k in range(3)]
    (outs[0] * _cu(gs[0])).sum().add((outs[2] * _cu(gs[1])).sum()).add((outs[3] * _cu(gs[2])).sum()).backward()
    dt, dn, st, sn = sref.grads64(cut(c["layers"]), cut(c["t"]), cut(c["normals"]), cut(c["ro"]), cut(c["rd"]), *gs)
    assert (np.abs(_np(tl.grad) - dt) <= summation_bound(np.abs(dt).max(), st)).all()
    assert (np.abs(_np(nl.grad) - dn) <= summation_bound(np.abs(dn).max(), sn)).all()
    # an empty window launches nothing
    with patched_C(shading_vectors_cuda=lambda *a: pytest.fail("launched")):
        e = r.shading_vectors(BIDX, torch.zeros((2, 0, 7, L), dtype=torch.int32, device="cuda"), torch.zeros((2, 0, 7, L), device="cuda"),
                              patch_min=_cu(pm))
    assert len(e) == 2 and tuple(e[0].shape) == (2, 0, 7, L, 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("which", ["all", "position", "normal", "reflection"])
def test_gradients_within_the_criterion(mode, L, which):
    c = _case(mode, L)
    _, r = _renderer(mode)
    shape = c["layers"].shape + (3,)
    gs = [np.random.default_rng(30 + k).standard_normal(shape).astype(f32) if which in ("all", name) else None
          for k, name in enumerate(("position", "normal", "reflection"))]
    calls = []
    real = _C.shading_vectors_backward_cuda

    def spy(*a):
        calls.append(a[5:])
        return real(*a)

    tl, nl = _cu(c["t"]).requires_grad_(True), _cu(c["normals"]).requires_grad_(True)
    with patched_C(shading_vectors_backward_cuda=spy):
        pos, view, nrm, refl = r.shading_vectors(BIDX, _cu(c["layers"]), tl, nl)
        assert not view.requires_grad and pos.requires_grad and refl.requires_grad
        loss = sum((o * _cu(g)).sum() for o, g in zip((pos, nrm, refl), gs) if g is not None)
        loss.backward()
        torch.cuda.synchronize()
    assert len(calls) == 1
    g_pos, g_nrm, g_refl, need_t, need_n = calls[0]
    assert [x is None for x in (g_pos, g_nrm, g_refl)] == [g is None for g in gs]        # left out of the loss: None upstream
    assert (need_t, need_n) == (gs[0] is not None, gs[1] is not None or gs[2] is not None)
    dt, dn, st, sn = sref.grads64(c["layers"], c["t"], c["normals"], c["ro"], c["rd"], *gs)
    live = c["layers"] >= 0
    for name, leaf, want, sabs, needed in (("t", tl, dt, st, need_t), ("normals", nl, dn, sn, need_n)):
        if not needed:
            assert leaf.grad is None and not want.any(), (which, name)               # not computed at all
            continue
        got = _np(leaf.grad).astype(np.float64)
        assert np.isfinite(got).all() and not got[~live].any() and not got[sabs == 0].any()
        gmax = np.abs(want).max()
        assert gmax > 0
        bound = summation_bound(gmax, sabs)
        print(f"shading_vectors {mode} L={L} {which} d{name}: worst error / bound {(np.abs(got - want) / bound).max():.3g}, "
              f"rel L_inf {np.abs(got - want).max() / gmax:.3g}")
        assert (np.abs(got - want) <= bound).all(), (mode, L, which, name)
    if need_n:                                                             # orthogonal to n
        got = _np(nl.grad).astype(np.float64)
        n64 = c["normals"].astype(np.float64)
        assert np.abs((got * n64).sum(-1)).max() <= 1e-5 * np.abs(got).max() * np.abs(n64).max()


def test_needs_input_grad_is_respected():
    c = _case("tensors", 4)
    _, r = _renderer("tensors")
    calls = []
    real = _C.shading_vectors_backward_cuda

    def spy(*a):
        calls.append(a[-2:])
        return real(*a)

    with patched_C(shading_vectors_backward_cuda=spy):
        outs = r.shading_vectors(BIDX, _cu(c["layers"]), _cu(c["t"]), _cu(c["normals"]))
        assert not any(o.requires_grad for o in outs)
        tl = _cu(c["t"]).requires_grad_(True)
        pos, view, nrm, refl = r.shading_vectors(BIDX, _cu(c["layers"]), tl, _cu(c["normals"]))
        assert pos.requires_grad
        (refl.sum() + nrm.sum()).backward()                                # reaches no input that wants a gradient
        assert not calls and tl.grad is None
        nl = _cu(c["normals"]).requires_grad_(True)
        pos, view, nrm, refl = r.shading_vectors(BIDX, _cu(c["layers"]), _cu(c["t"]), nl)
        (pos.sum() + refl.sum()).backward()
        assert calls == [(False, True)] and nl.grad is not None
        pos, view = r.shading_vectors(BIDX, _cu(c["layers"]), tl)
        (pos * pos).sum().backward()
        assert calls[-1] == (True, False) and tl.grad is not None


def test_empty_and_invalid_slots():
    c = _case("tensors", 4)
    _, r = _renderer("tensors")
    layers, t, n = c["layers"].copy(), c["t"].copy(), c["normals"].copy()
    live = np.argwhere(layers >= 0)
    assert len(live) > 40
    pick = lambda k: tuple(live[k])
    layers[pick(0)] = -7
    t[pick(1)], t[pick(2)], t[pick(3)], t[pick(4)] = np.nan, np.inf, -np.inf, -0.0
    n[pick(5)] = (-0.0, 0.0, -0.0)
    n[pick(6)] = (np.nan, 1.0, 0.0)
    n[pick(7)] = (1.0, -np.inf, 0.0)
    n[pick(8)] = (3e38, 3e38, 0.0)
    n[pick(9)] = (1e-30, 0.0, 0.0)                                         # nx nx underflows: nl == 0
    t[pick(10)] = 3e38                                                     # finite: position may overflow, as the formula says
    want = sref.forward32(layers, t, n, c["ro"], c["rd"])
    tl, nl = _cu(t).requires_grad_(True), _cu(n).requires_grad_(True)
    got = r.shading_vectors(BIDX, _cu(layers), tl, nl)
    _same(got, want, "invalid slots")
    for k in range(4):
        assert not any(_np(o)[pick(k)].any() for o in got)
    assert _np(got[0])[pick(4)].any() and _np(got[2])[pick(4)].any()
    for k in range(5, 10):
        assert not _np(got[2])[pick(k)].any() and not _np(got[3])[pick(k)].any() and _np(got[1])[pick(k)].any()
    gs = [np.random.default_rng(50 + k).standard_normal(n.shape).astype(f32) for k in range(3)]
    keep = np.ones(layers.shape, bool)
    keep[pick(10)] = False                                                 # (an infinite position times its gradient: not in the loss)
    loss = sum((torch.where(_cu(keep)[..., None], o, torch.zeros_like(o)) * _cu(g)).sum() for o, g in zip((got[0], got[2], got[3]), gs))
    loss.backward()
    dt, dn = _np(tl.grad), _np(nl.grad)
    assert np.isfinite(dt).all() and np.isfinite(dn).all()
    for k in range(4):
        assert dt[pick(k)] == 0 and not dn[pick(k)].any()
    for k in range(5, 10):
        assert dt[pick(k)] != 0 and not dn[pick(k)].any()
    gk = [np.where(keep[..., None], g, 0).astype(f32) for g in gs]
    wt, wn, st, sn = sref.grads64(layers, t, n, c["ro"], c["rd"], *gk)
    assert (np.abs(dt - wt) <= summation_bound(np.abs(wt).max(), st)).all()
    assert (np.abs(dn - wn) <= summation_bound(np.abs(wn).max(), sn)).all()


def test_argument_checks():
    c = _case("tensors", 4)
    ts, r = _renderer("tensors")
    rl, t, n = _cu(c["layers"]), _cu(c["t"]), _cu(c["normals"])
    ro, rd = _cu(c["ro"]), _cu(c["rd"])
    ok = _C.shading_vectors_cuda(rl, t, n, ro, rd)
    assert len(ok) == 4
    for args, name in (((rl[0], t, n, ro, rd), "render_layers"), ((rl.long(), t, n, ro, rd), "render_layers"),
                       ((rl, t[..., :2], n, ro, rd), "t must"), ((rl, t.double(), n, ro, rd), "t: expected"),
                       ((rl, t, n[..., :2], ro, rd), "normals"), ((rl, t, n.half(), ro, rd), "normals"),
                       ((rl, t, n, ro[:1], rd), "image_ray_o"), ((rl, t, n, ro, rd[:, :5]), "image_ray_o/image_ray_d"),
                       ((rl, t, n, ro, rd.double()), "image_ray_d")):
        with pytest.raises(RuntimeError, match=name):
            _C.shading_vectors_cuda(*args)
    with pytest.raises(RuntimeError, match="g_normal"):
        _C.shading_vectors_backward_cuda(rl, t, n, ro, rd, None, ok[0][..., :2], None, True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.shading_vectors_cuda(rl.cpu(), t.cpu(), n.cpu(), ro.cpu(), rd.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.shading_vectors(BIDX, rl, t.cpu())
    with pytest.raises(ValueError, match="render_layers"):
        r.shading_vectors(BIDX, rl[0], t[0])
    with pytest.raises(ValueError, match="patch_min"):
        r.shading_vectors(BIDX, rl[:, :10], t[:, :10])
    with pytest.raises(ValueError, match="patch_min"):
        r.shading_vectors(BIDX, rl[:, :10], t[:, :10], patch_min=torch.zeros((3, 2), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="negative"):
        r.shading_vectors(BIDX, rl[:, :10], t[:, :10], patch_min=torch.tensor([[0, -1], [0, 0]], dtype=torch.int32, device="cuda"))
    with pytest.raises(AssertionError, match="exceed"):
        r.shading_vectors(BIDX, rl[:, :10], t[:, :10], patch_min=torch.tensor([[0, 15], [0, 0]], dtype=torch.int32, device="cuda"))
    with _C.analytic_rays(torch.zeros((2, 32), device="cuda"), W + 1, H):
        with pytest.raises(RuntimeError, match="analytic_rays"):
            _C.shading_vectors_cuda(rl, t, n, ro, rd)
    # no gradient wanted, or none arriving: nothing runs
    assert _C.shading_vectors_backward_cuda(rl, t, n, ro, rd, ok[0], ok[0], ok[0], False, False) == (None, None)
    assert _C.shading_vectors_backward_cuda(rl, t, n, ro, rd, None, None, None, True, True) == (None, None)
    assert _C.shading_vectors_backward_cuda(rl, t, None, ro, rd, None, ok[0], None, True, True) == (None, None)
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    p = _C._ptr
    B, Hh, Ww, L = rl.shape
    outs = [torch.empty_like(o) for o in ok]
    good = (p(rl), p(t), p(n), p(ro), p(rd), None)
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, L, 0, None, *good, *(p(o) for o in outs), None) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, ok))
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, -1, 0, None, *good, *(p(o) for o in outs), None) == 1
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, L, 4, None, *good, *(p(o) for o in outs), None) == 1
    assert b"flag" in lib.dm2_last_error()
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, L, _C.DM2_FLAG_ANALYTIC_RAYS, None, *good, *(p(o) for o in outs), None) == 1   # no ray_cam
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, L, 0, None, p(rl), p(t), p(n), None, p(rd), None, *(p(o) for o in outs), None) == 1
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, L, 0, None, None, p(t), p(n), p(ro), p(rd), None, *(p(o) for o in outs), None) == 1
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, L, 0, None, *good, p(outs[0]), None, p(outs[2]), p(outs[3]), None) == 1
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, L, 0, None, *good, p(outs[0]), p(outs[1]), None, None, None) == 1
    win = _C.Window()
    win.patch_min, win.full_W, win.full_H = None, Ww - 1, Hh
    import ctypes
    assert lib.dm2_shading_vectors_window(B, Hh, Ww, L, 0, ctypes.byref(win), *good, *(p(o) for o in outs), None) == 1
    assert lib.dm2_shading_vectors_backward_window(B, Hh, Ww, L, 0, None, p(rl), p(t), None, p(ro), p(rd), None, p(ok[0]), None, None,
                                                   None, p(outs[0]), None) == 1      # dL_dnormals without normals
    assert lib.dm2_shading_vectors_backward_window(B, Hh, Ww, L, 0, None, *good, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()


def _module_pipeline(mode):
    """-> run(ours, view_in=None) -> (verts.grad, cube.grad, view, image): the pipeline of test_module_path_end_to_end on a tet
    lattice, with this package's two ops (ours) or with the torch lines they replace."""
    Wm, Hm, L, N, C = 80, 64, 4, 16, 3
    # + 93, not the next free seed + 92: that lattice has a slot whose reflection lies on a cube edge to the bit, where the
    # torch route's own gradient is not reproducible (see the precondition in test_module_path_end_to_end).  Should
    # scenes.tet_lattice ever change what a seed gives, that precondition fails first: pick a seed that meets it again.
    ts = scenes.tet_lattice(Wm, Hm, 4, seed=scenes.SEED_BASE + 93, num_cams=2).to("cuda")
    r = dm2.LayeredRenderer(ts.mv, ts.proj, Wm, Hm, "cuda", analytic_rays=mode == "analytic")
    faces, P = ts.faces, ts.verts.shape[0]
    gen = torch.Generator().manual_seed(13)
    # an environment that is smooth on the sphere (an affine function of the texel's direction): the two routes differ in the
    # last bits of the reflection, and across a texel border of a random cube that alone would change a slot's gradient
    import texture_cube_ref as cref
    centre = lambda k: 2.0 * (k + 0.5) / N - 1.0
    pts = np.array([[[cref._point(f, centre(i), centre(j)) for i in range(N)] for j in range(N)] for f in range(6)])
    dirs = torch.from_numpy(pts / np.linalg.norm(pts, axis=-1, keepdims=True)).float()
    tex0 = (dirs @ torch.randn((3, C), generator=gen) + torch.randn((C,), generator=gen)).cuda()
    alpha0 = torch.rand((faces.shape[0],), generator=gen).cuda() * 0.8 + 0.1
    bg = torch.tensor([0.2, -0.1, 0.5]).cuda()
    wgt = torch.randn((2, Hm, Wm, C), generator=gen).cuda()
    adjacency = r.vertex_adjacency(faces, P)

    def torch_normals(verts):
        fl = faces.long()
        p0, p1, p2 = verts[fl[:, 0]], verts[fl[:, 1]], verts[fl[:, 2]]
        fn = torch.cross(p1 - p0, p2 - p0, dim=-1)
        vn = torch.zeros_like(verts)
        for k in range(3):
            vn = vn.index_add(0, fl[:, k], fn)
        return torch.nn.functional.normalize(vn, dim=-1)

    def run(ours, view_in=None):
        verts, tex = ts.verts.clone().requires_grad_(True), tex0.clone().requires_grad_(True)
        layers, cnt, bary, t = r.rasterize(BIDX, verts, faces, L)
        vn = r.vertex_normals(verts, faces, adjacency) if ours else torch_normals(verts)
        nimg = r.interpolate(layers, bary, vn, faces)
        if ours:
            pos, view, nrm, refl = r.shading_vectors(BIDX, layers, t, nimg)
        else:
            view = view_in if view_in is not None else \
                (-r.ray_d[BIDX])[:, :, :, None, :].expand(-1, -1, -1, L, -1) * (layers >= 0)[..., None]
            nrm = torch.nn.functional.normalize(nimg, dim=-1)
            refl = 2.0 * (nrm * view).sum(-1, keepdim=True) * nrm - view
        shaded = r.texture(refl, tex, layers, boundary_mode="cube")
        out, acc = r.composite(shaded, alpha0, layers, bg)
        (out * wgt).sum().backward()
        torch.cuda.synchronize()
        assert int(cnt.sum()) > 3000
        return verts.grad, tex.grad, view.detach(), out.detach(), refl.detach()[layers >= 0]
    return run


@pytest.mark.parametrize("mode", MODES)
def test_module_path_end_to_end(mode):
    """rasterize -> interpolate(vertex_normals(verts, faces)) -> shading_vectors -> texture(reflection, cube) -> composite ->
    backward: finite, non-zero verts.grad and cube gradient, and verts.grad within 1e-3 of its maximum (test_gpu_camera_grad.py's
    bar between a fused and a torch route) of the same pipeline with the two ops replaced by their torch lines: index_add_
    normals with normalize, and the reflection formula (under analytic rays fed shading_vectors' own view)."""
    run = _module_pipeline(mode)
    gv, gt, view, out, refl = run(True)
    for x in (gv, gt):
        assert x is not None and torch.isfinite(x).all() and x.abs().max() > 0
    # what the comparison of two fp32 routes presupposes of the scene: no filled slot's reflection within a few ulp of a cube
    # edge (its two largest |components| equal).  There the lookup's derivative jumps by O(1 / N) of itself, and the last bits --
    # which index_add_'s atomics change from run to run -- choose the face.  (seed SEED_BASE + 92 has one such slot, x == z to
    # the bit, and the torch route alone then gives one of two gradients, 1.5e-3 of the maximum apart.)
    top2 = refl.abs().sort(dim=-1).values[:, 1:]
    assert int(((top2[:, 1] - top2[:, 0]) <= 1e-6 * top2[:, 1]).sum()) == 0
    wv, wt, _, wout, _ = run(False, view if mode == "analytic" else None)
    ev = float((gv - wv).abs().max() / wv.abs().max())
    et = float((gt - wt).abs().max() / wt.abs().max())
    eo = float((out - wout).abs().max())
    print(f"module path {mode}: verts.grad {ev:.3g}, tex.grad {et:.3g} of their maxima against the torch lines; image {eo:.3g}")
    assert ev <= 1e-3 and et <= 1e-3
