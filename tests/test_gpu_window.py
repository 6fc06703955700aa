"""Render windows on the deferred path (include/dm2_hip.h: dm2_window) on the GPU against the windowed restatements of
tests/window_ref.py: Renderer.rasterize, LayeredRenderer.generate, Renderer.coverage and LayeredRenderer.render with
``patch_min``, forward bit for bit, gradients at the full-frame tests' bars, analytic rays, the backward tables' overflow route
at an offset, the pipeline rasterize -> interpolate -> texture -> coverage -> composite on a window, and the argument checks."""
import numpy as np
import pytest
import torch

import coverage_ref as cref
import generate_ref as G
import layer_composite_ref as lref
import rasterize_ref as rref
import tet_scenes as S
import window_ref as wref
from util import GRAD_TOL, rel_linf, scenes, spy_library, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
OUTS = ("layers", "cnt", "bary", "t")
LS = (1, 4, 17)
WINS = ("a", "b", "c", "d", "e")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what):
    got = _np(got) if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))


def _rasterize(s, fe, L, win=None):
    """_C.rasterize_layers_cuda on scene ``s``: the full frame, or the window (patch_min, pw, ph) with its cut of the rays."""
    fixed = (_cu(s["verts"]), _cu(s["faces"]), _cu(fe), _cu(s["verts_ndc"]), _cu(s["verts_image"]))
    if win is None:
        return _C.rasterize_layers_cuda(s["W"], s["H"], *fixed, _cu(s["ray_o"]), _cu(s["ray_d"]), L)
    pm, pw, ph = win
    ro, rd = wref.rays(s, pm, pw, ph)
    with _C.window(_cu(pm), s["W"], s["H"]):
        return _C.rasterize_layers_cuda(pw, ph, *fixed, _cu(ro), _cu(rd), L)


# ---- rasterize -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wref.SCENES)
@pytest.mark.parametrize("win", WINS)
def test_rasterize_window_bit_equal_to_restatement(name, win):
    """L = 1, 4, 17 (k_rasterize<1>, <4> and <16> with a second pass), with and without existence flags: ids, counts,
    barycentrics and t of the window bit-equal to the windowed restatement; (a) also to the call without a window, (b) also to the
    crop of the full-frame GPU result."""
    s = wref.scene2(name)
    pm, pw, ph = wref.windows(s["W"], s["H"])[win]
    for fe in (None, s["fe"]):
        x = wref.intersect(s, pm, pw, ph, fe)
        for L in LS:
            got = _rasterize(s, fe, L, (pm, pw, ph))
            want = rref.select(x, L)
            for k, g in zip(OUTS, got):
                _same(g, want[k], (name, win, L, fe is None, k))
            if win in ("a", "b"):
                full = _rasterize(s, fe, L)
                for k, g, f in zip(OUTS, got, full):
                    _same(g, wref.cut(_np(f), pm, pw, ph), (name, win, L, k, "full frame"))
        if win != "e":
            assert want["cnt"].max() > 1


def _module_scene(analytic, name="aligned"):
    """Tet scene ``name`` on the GPU with a LayeredRenderer that computes its rays (analytic) or reads the very same rays, as
    the oracle computes them, from tensors."""
    from oracle import cpu as orc
    ts, _ = S.case(name)
    scd = ts.to("cuda")
    lr = S.renderer(ts, "cuda", analytic_rays=analytic)
    if not analytic:
        ref = S.renderer(ts, "cuda", analytic_rays=True)
        cam = ref.ray_cam.cpu().numpy()
        ro, rd = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), ts.width, ts.height)
        lr.ray_o, lr.ray_d = _cu(ro), _cu(rd)
    return ts, scd, lr


def _material(P, F, seed=7):
    g = np.random.RandomState(seed)
    return dict(verts_color=g.uniform(0, 1, (P, 3)).astype(f32), faces_opacity=g.uniform(0.05, 0.95, F).astype(f32),
                faces_intense=g.uniform(0.5, 1.5, (2, F)).astype(f32), background=np.array([0.1, 0.3, 0.7], f32))


@pytest.mark.parametrize("win", ["a", "c", "d"])
def test_analytic_rays_bit_equal_to_the_ray_tensor_path(win):
    """rasterize (with its backward), generate and render on a window: the module that computes each pixel's ray from the
    absolute pixel and the frame's size gives the bits of the module that reads the window's cut of the oracle's analytic rays.
    (render and generate use the origin for nothing else.)"""
    bidx, L = [1, 0], 5
    res = []
    for analytic in (True, False):
        ts, scd, lr = _module_scene(analytic)
        pm, pw, ph = wref.windows(ts.width, ts.height)[win]
        kw = dict(patch_min=_cu(pm), patch_width=pw, patch_height=ph)
        v = scd.verts.clone().requires_grad_(True)
        ras = lr.rasterize(bidx, v, scd.faces, L, faces_existence=scd.faces_existence, **kw)
        gb = torch.randn(ras[2].shape, generator=torch.Generator().manual_seed(7)).cuda()
        gt = torch.randn(ras[3].shape, generator=torch.Generator().manual_seed(8)).cuda()
        ((ras[2] * gb).sum() + (ras[3] * gt).sum()).backward()
        gen = lr.generate(bidx, scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, scd.faces_existence, L, **kw)
        m = {k: _cu(a) for k, a in _material(ts.verts.shape[0], ts.faces.shape[0]).items()}
        ren = lr.render(bidx, gen[0], scd.verts, scd.faces, m["verts_color"], m["faces_opacity"], m["faces_intense"],
                        m["background"], return_alpha=True, patch_min=_cu(pm))
        res.append(([_np(x) for x in ras + gen + ren], _np(v.grad)))
    assert lr.ray_o is not None
    for k, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        assert a.shape[1:3] == (ph, pw)
        assert np.array_equal(_bits(a), _bits(b)), (win, k)
    assert (res[0][0][1] > 0).sum() > 0.2 * res[0][0][1].size and (res[0][0][5] > 0).any()
    assert rel_linf(res[0][1], res[1][1]) <= 2e-6            # (test_gpu_rasterize.py's bar for the same comparison)


def test_rasterize_module_window_equals_its_own_inputs_restated():
    """Renderer.rasterize(patch_min=...) with both host preps and analytic rays, window (c): the op gets the window's size, the
    window's rays and the origins, and its result is the windowed restatement of the very inputs it got; (a) through the module
    is, bit for bit, the call without patch_min."""
    from oracle import cpu as orc
    ts, _ = S.case("aligned")
    W, H, bidx, L = ts.width, ts.height, [0, 1], 4
    scd = ts.to("cuda")
    wins = wref.windows(W, H)
    pm, pw, ph = wins["c"]
    seen = []
    real = _C.rasterize_layers_cuda

    def spy(*a):
        out = real(*a)
        seen.append(([_np(x) if torch.is_tensor(x) else x for x in a], getattr(_C._tls, "window", None), out))
        return out
    _C.rasterize_layers_cuda = spy
    try:
        for kw in (dict(fused_prep=False), dict(fused_prep=True), dict(analytic_rays=True)):
            lr = dm2.LayeredRenderer(scd.mv, scd.proj, W, H, "cuda", **kw)
            out = lr.rasterize(bidx, scd.verts, scd.faces, L, faces_existence=scd.faces_existence, patch_min=_cu(pm), patch_width=pw,
                               patch_height=ph)
            a, w, _ = seen[-1]
            assert (a[0], a[1]) == (pw, ph) and w[1:] == (W, H) and np.array_equal(_np(w[0]), pm)
            if kw.get("analytic_rays"):
                cam = lr.ray_cam.cpu().numpy()
                ro, rd = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), W, H)
            else:
                ro, rd = _np(lr.ray_o[bidx]), _np(lr.ray_d[bidx])
                assert np.array_equal(a[7], wref.cut(ro, pm, pw, ph)) and np.array_equal(a[8], wref.cut(rd, pm, pw, ph))
            s = dict(verts=a[2], faces=a[3], verts_ndc=a[5], verts_image=a[6], ray_o=ro, ray_d=rd)
            want = rref.select(wref.intersect(s, pm, pw, ph, a[4]), L)
            for k, g in zip(OUTS, out):
                _same(g, want[k], (kw, k))
            pa, wa, ha = wins["a"]
            full = lr.rasterize(bidx, scd.verts, scd.faces, L, faces_existence=scd.faces_existence)
            assert seen[-1][1] is None
            deg = lr.rasterize(bidx, scd.verts, scd.faces, L, faces_existence=scd.faces_existence, patch_min=_cu(pa), patch_width=wa,
                               patch_height=ha)
            assert seen[-1][1] is not None
            for k, g, f in zip(OUTS, deg, full):
                _same(g, _np(f), (kw, k, "degenerate window"))
    finally:
        _C.rasterize_layers_cuda = real


def test_empty_windows_launch_nothing():
    """(f): pw == 0 (and ph == 0): empty tensors of the window's shape, and no entry point of the library is called."""
    ts, scd, lr = _module_scene(False)
    B, L, F = 2, 3, ts.faces.shape[0]
    m = {k: _cu(a) for k, a in _material(ts.verts.shape[0], F).items()}
    calls = []
    lib = _C.load_library()
    names = [n for n in _C.EXPORTS if n not in ("dm2_abi_version", "dm2_last_error")]
    wrap = {n: (lambda *a, _n=n: calls.append(_n) or getattr(lib, _n)(*a)) for n in names}
    for pw, ph in ((0, 13), (9, 0)):
        pm = _cu(wref.windows(ts.width, ts.height)["f"][0])
        kw = dict(patch_min=pm, patch_width=pw, patch_height=ph)
        with spy_library(**wrap):
            ras = lr.rasterize([1, 0], scd.verts, scd.faces, L, **kw)
            gen = lr.generate([1, 0], scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, scd.faces_existence, L, **kw)
            cov = lr.coverage([1, 0], gen[0], scd.verts, scd.faces, patch_min=pm)
            ren = lr.render([1, 0], gen[0], scd.verts, scd.faces, m["verts_color"], m["faces_opacity"], m["faces_intense"],
                            m["background"], return_alpha=True, return_face_weights=True, patch_min=pm)
        assert not calls, calls
        assert [tuple(x.shape) for x in ras] == [(B, ph, pw, L), (B, ph, pw), (B, ph, pw, L, 3), (B, ph, pw, L)]
        assert [x.dtype for x in ras] == [torch.int32, torch.int32, torch.float32, torch.float32]
        assert [tuple(x.shape) for x in gen] == [(B, ph, pw, L), (B, ph, pw)] and gen[0].dtype == torch.int32
        assert tuple(cov.shape) == (B, ph, pw, L) and cov.dtype == torch.float32
        assert [tuple(x.shape) for x in ren] == [(B, ph, pw, 3), (B, ph, pw), (B, ph, pw), (B, F)] and not ren[3].any()


# ---- generate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["aligned", "holes"])
@pytest.mark.parametrize("walk", ["records", "legacy"])
def test_generate_window_equals_the_windowed_oracle(name, walk):
    """Both tet walks over windows (a)-(e): ids and counts equal the oracle's layer generator on the oracle's binning of the
    window and the window's rays; (a) equals the call without patch_min."""
    ts, _ = S.case(name)
    scd = ts.to("cuda")
    lr = S.renderer(ts, "cuda")
    bidx, L = [1, 0], 4
    inp = G.inputs(lr, scd.verts, bidx)
    args = (bidx, scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, scd.faces_existence, L)
    old = _C.set_flags(_C.DM2_FLAG_LEGACY_KERNELS if walk == "legacy" else 0)
    try:
        for win, (pm, pw, ph) in wref.windows(ts.width, ts.height).items():
            if win == "f":
                continue
            layers, cnt = lr.generate(*args, patch_min=_cu(pm), patch_width=pw, patch_height=ph)
            wl, wc = wref.generate(ts, inp["ndc"], inp["img"], inp["ro"], inp["rd"], pm, pw, ph, L)
            _same(layers, wl, (name, walk, win, "layers"))
            _same(cnt, wc, (name, walk, win, "cnt"))
            if win == "a":
                fl, fcnt = lr.generate(*args)
                _same(layers, _np(fl), "degenerate"); _same(cnt, _np(fcnt), "degenerate")
            if win in ("a", "c"):
                assert (wc > 0).sum() > 50 and wc.max() > 1, (name, win)
    finally:
        _C.set_flags(old)


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def _coverage_case(name, win, L=4):
    """The windowed restatement's lists of a scene at L layers, for coverage: dict(pm, W, H, layers (window), verts_image, faces)."""
    s = wref.scene2(name)
    pm, pw, ph = wref.windows(s["W"], s["H"])[win]
    return dict(pm=pm, W=s["W"], H=s["H"], layers=wref.rasterize32(s, pm, pw, ph, L)["layers"], verts_image=s["verts_image"],
                faces=s["faces"])


@pytest.mark.parametrize("name", wref.SCENES)
@pytest.mark.parametrize("win", WINS)
def test_coverage_window_bit_equal_to_restatement(name, win):
    """Temperatures 1, 0.5 and 0 (L = 4: the vector id path; L = 3: the scalar one): the window's coverage is the crop of
    coverage32 on the layers embedded in a frame of -1."""
    for L in (4, 3):
        c = _coverage_case(name, win, L)
        for t in cref.TEMPERATURES:
            info, want = wref.coverage32(c["layers"], c["pm"], c["W"], c["H"], c["verts_image"], c["faces"], t)
            with _C.window(_cu(c["pm"]), c["W"], c["H"]):
                got = _C.coverage_cuda(_cu(c["layers"]), _cu(c["verts_image"]), _cu(c["faces"]), t)
            _same(got, want, (name, win, L, t))
        if win in ("a", "b", "c"):
            assert info["partial"].sum() > 100 and info["full"].sum() > 0, (name, win)


@pytest.mark.parametrize("name", wref.SCENES)
def test_coverage_window_backward(name):
    """Window (c): dL/dverts_image within GRAD_TOL of grad_image64 on the embedded layers, and of the full-frame op's backward
    fed the upstream gradient embedded in zeros; exact zeros where the reference has zeros."""
    c = _coverage_case(name, "c")
    g = cref.upstream(c["layers"].shape, 5)
    frame_layers = wref.embed(c["layers"], c["pm"], c["W"], c["H"], -1)
    frame_g = wref.embed(g, c["pm"], c["W"], c["H"], 0)
    vi, fc = _cu(c["verts_image"]), _cu(c["faces"])
    for t in (1.0, 0.5):
        want = cref.grad_image64(frame_layers, c["verts_image"], c["faces"], t, frame_g)
        with _C.window(_cu(c["pm"]), c["W"], c["H"]):
            got = _np(_C.coverage_backward_cuda(_cu(c["layers"]), vi, fc, t, _cu(g)))
        full = _np(_C.coverage_backward_cuda(_cu(frame_layers), vi, fc, t, _cu(frame_g)))
        assert np.isfinite(got).all() and np.abs(want).max() > 0 and not got[want == 0].any()
        print(name, t, rel_linf(got, want), rel_linf(got, full))
        assert rel_linf(got, want) <= GRAD_TOL and rel_linf(got, full) <= GRAD_TOL, (name, t)
    with _C.window(_cu(c["pm"]), c["W"], c["H"]):
        assert _C.coverage_backward_cuda(_cu(c["layers"]), vi, fc, 0.0, _cu(g)) is None


# ---- render --------------------------------------------------------------------------------------------------------------------
def _render_inputs(name, win, L=5):
    """The windowed restatement's lists of ``name`` with a material: (inputs of forward32 with the WINDOW's layers and the
    FRAME's rays, pm, W, H)."""
    s = wref.scene2(name)
    pm, pw, ph = wref.windows(s["W"], s["H"])[win]
    layers = wref.rasterize32(s, pm, pw, ph, L)["layers"].copy()
    layers[:, ::3, :, 1] = layers[:, ::3, :, 0]                            # a face twice in a pixel's list
    layers[:, 1::4, ::3, 0] = s["faces"].shape[0] + 2                      # ids out of range
    inp = dict(render_layers=layers, verts=s["verts"], faces=s["faces"], verts_ndc=s["verts_ndc"], ray_o=s["ray_o"], ray_d=s["ray_d"],
               **_material(s["verts"].shape[0], s["faces"].shape[0]))
    return inp, pm, s["W"], s["H"]


ARGS = ("render_layers", "verts", "faces", "verts_color", "faces_opacity", "faces_intense", "verts_ndc", "background")


def _composite_op(inp, pm, W, H, weights=False):
    """_C.composite_layers_cuda on the window's layers and the window's cut of the rays -> outputs, device args."""
    rl = inp["render_layers"]
    ro, rd = wref.cut(inp["ray_o"], pm, rl.shape[2], rl.shape[1]), wref.cut(inp["ray_d"], pm, rl.shape[2], rl.shape[1])
    args = [_cu(inp[k]) for k in ARGS] + [_cu(ro), _cu(rd)]
    with _C.window(_cu(pm), W, H), _C.face_weights_output(weights):
        return _C.composite_layers_cuda(*args), args


@pytest.mark.parametrize("name", wref.SCENES)
@pytest.mark.parametrize("win", WINS)
def test_render_window_bit_equal_to_restatement(name, win):
    """dm2_layers_composite under a window: colour, raw depth, final T and n_contrib of the window are the crop of forward32 on the
    layers embedded in a frame of -1, bit for bit; so with face weights, which sum to the window's blends."""
    from face_weights_ref import layered_face_weights64
    from test_gpu_face_weights import check_weights
    inp, pm, W, H = _render_inputs(name, win)
    fwd, want = wref.composite32(inp, pm, W, H)
    for weights in (False, True):
        out, _ = _composite_op(inp, pm, W, H, weights)
        for k, g in zip(("color", "depth_raw", "final_T", "n_contrib"), out):
            _same(g, want[k].reshape(tuple(g.shape)), (name, win, k, weights))
    if win != "e":
        assert fwd["blend"].sum() > 200
        check_weights(out[4], layered_face_weights64(fwd, inp["faces_opacity"], inp["faces"].shape[0]))


def test_render_module_window():
    """LayeredRenderer.render(patch_min=...) with return_alpha and return_face_weights on window (c) of generate's own window
    layers: colour bit-equal to the embedded restatement, depth and alpha the module's own fp32 maps of its raw depth and final
    T, face weights within their bar; the gradients of colour, depth and alpha against float64 at GRAD_TOL and against the
    full-frame module fed the embedded layers and upstream gradients embedded in zeros."""
    from face_weights_ref import layered_face_weights64
    from test_gpu_face_weights import check_weights
    ts, _ = S.case("holes")
    scd = ts.to("cuda")
    lr = S.renderer(ts, "cuda")
    bidx, L = [1, 0], 6
    W, H = ts.width, ts.height
    pm, pw, ph = wref.windows(W, H)["c"]
    layers, cnt = lr.generate(bidx, scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, scd.faces_existence, L,
                              patch_min=_cu(pm), patch_width=pw, patch_height=ph)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    mat = _material(P, F)
    inp = G.inputs(lr, scd.verts, bidx)
    full_in = dict(render_layers=_np(layers), verts=_np(ts.verts), faces=_np(ts.faces), verts_ndc=inp["ndc"], ray_o=inp["ro"],
                   ray_d=inp["rd"], **mat)
    fwd, want = wref.composite32(full_in, pm, W, H)
    gen = torch.Generator().manual_seed(3)
    gc, gd, ga = (torch.randn(s, generator=gen) for s in ((2, ph, pw, 3), (2, ph, pw), (2, ph, pw)))
    names = ("verts_color", "faces_opacity", "faces_intense")
    grads = []
    for windowed in (True, False):
        leaves = [_cu(mat[k]).requires_grad_(True) for k in names]
        rl = layers if windowed else _cu(wref.embed(_np(layers), pm, W, H, -1))
        kw = dict(patch_min=_cu(pm)) if windowed else {}
        color, depth, alpha, fw = lr.render(bidx, rl, scd.verts, scd.faces, *leaves, _cu(mat["background"]), return_alpha=True,
                                            return_face_weights=True, **kw)
        up = [g if windowed else wref.embed(g.numpy(), pm, W, H, 0) for g in (gc, gd, ga)]
        up = [_cu(g) if isinstance(g, np.ndarray) else g.cuda() for g in up]
        ((color * up[0]).sum() + (depth * up[1]).sum() + (alpha * up[2]).sum()).backward()
        grads.append([_np(x.grad) for x in leaves])
        if windowed:
            _same(color, want["color"], "color")
            _same(depth, _np(1.0 - (_cu(want["depth_raw"]) + 1.0) / 2.0), "depth")
            _same(alpha, _np(1.0 - _cu(want["final_T"])), "alpha")
            check_weights(fw, layered_face_weights64(fwd, mat["faces_opacity"], F))
    assert fwd["blend"].sum() > 500
    # colour, depth and alpha in the loss: the window against the full-frame module
    for a, b in zip(*grads):
        assert np.abs(b).max() > 0 and rel_linf(a, b) <= GRAD_TOL, rel_linf(a, b)
    # colour and depth in the loss (the float64 restatement has no alpha output): against float64, depth = 1 - (raw + 1) / 2
    leaves = [_cu(mat[k]).requires_grad_(True) for k in names]
    color, depth = lr.render(bidx, layers, scd.verts, scd.faces, *leaves, _cu(mat["background"]), patch_min=_cu(pm))
    ((color * gc.cuda()).sum() + (depth * gd.cuda()).sum()).backward()
    frame_gc = wref.embed(gc.numpy(), pm, W, H, 0).astype(np.float64)
    frame_gd = wref.embed(gd.numpy(), pm, W, H, 0).astype(np.float64) * -0.5          # d(depth) / d(raw depth)
    w64 = lref.grads64(fwd, full_in["faces"], mat["verts_color"], mat["faces_opacity"], mat["faces_intense"], inp["ndc"],
                       mat["background"], frame_gc, frame_gd)
    for k, x in zip(names, leaves):
        e = rel_linf(_np(x.grad), w64[k])
        print("render window", k, e)
        assert e <= GRAD_TOL, (k, e)


@pytest.mark.parametrize("name", wref.SCENES)
def test_render_window_backward_op(name):
    """dm2_layers_composite_backward on window (c): the four gradients within GRAD_TOL of float64 on the embedded layers
    and of the full-frame op fed upstream gradients embedded in zeros."""
    inp, pm, W, H = _render_inputs(name, "c")
    fwd, _ = wref.composite32(inp, pm, W, H)
    out, args = _composite_op(inp, pm, W, H)
    gen = torch.Generator().manual_seed(11)
    gc, gd = torch.randn(out[0].shape, generator=gen), torch.randn(out[1].shape, generator=gen)
    with _C.window(_cu(pm), W, H):
        got = _C.composite_layers_backward_cuda(*args, out[3], gc.cuda(), gd.cuda())
    frame = dict(inp, render_layers=wref.embed(inp["render_layers"], pm, W, H, -1))
    fargs = [_cu(frame[k]) for k in ARGS] + [_cu(inp["ray_o"]), _cu(inp["ray_d"])]
    fout = _C.composite_layers_cuda(*fargs)
    fgc, fgd = wref.embed(gc.numpy(), pm, W, H, 0), wref.embed(gd.numpy(), pm, W, H, 0)
    full = _C.composite_layers_backward_cuda(*fargs, fout[3], _cu(fgc), _cu(fgd))
    want = lref.grads64(fwd, inp["faces"], inp["verts_color"], inp["faces_opacity"], inp["faces_intense"], inp["verts_ndc"],
                        inp["background"], fgc.astype(np.float64), fgd.astype(np.float64))
    for k, g, f in zip(("verts_color", "faces_opacity", "verts_ndc", "faces_intense"), got, full):
        g = _np(g)
        assert np.isfinite(g).all() and np.abs(want[k]).max() > 0
        print(name, k, rel_linf(g, want[k]), rel_linf(g, _np(f)))
        assert rel_linf(g, want[k]) <= GRAD_TOL and rel_linf(g, _np(f)) <= GRAD_TOL, (name, k)


# ---- rasterize's backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wref.SCENES)
@pytest.mark.parametrize("L", [4, 17])
def test_rasterize_window_backward(name, L):
    """Window (c): verts.grad within GRAD_TOL of float64 autograd over the listed pairs with the window's rays, and of the
    full-frame backward fed the layers embedded in -1 and the upstream gradients embedded in zeros."""
    s = wref.scene2(name)
    pm, pw, ph = wref.windows(s["W"], s["H"])["c"]
    layers, cnt, bary, t = _rasterize(s, s["fe"], L, (pm, pw, ph))
    gen = torch.Generator().manual_seed(L)
    gb, gt = torch.randn(bary.shape, generator=gen), torch.randn(t.shape, generator=gen)
    ro, rd = wref.rays(s, pm, pw, ph)
    verts, faces = _cu(s["verts"]), _cu(s["faces"])
    frame_layers = _cu(wref.embed(_np(layers), pm, s["W"], s["H"], -1))
    for g_b, g_t in ((gb, gt), (gb, None), (None, gt)):
        with _C.window(_cu(pm), s["W"], s["H"]):
            got = _np(_C.rasterize_layers_backward_cuda(layers, verts, faces, _cu(ro), _cu(rd), None if g_b is None else g_b.cuda(),
                                                        None if g_t is None else g_t.cuda()))
        want = rref.grads64(s["verts"], s["faces"], layers.cpu(), ro, rd, g_b, g_t)
        fb = None if g_b is None else _cu(wref.embed(g_b.numpy(), pm, s["W"], s["H"], 0))
        ft = None if g_t is None else _cu(wref.embed(g_t.numpy(), pm, s["W"], s["H"], 0))
        full = _np(_C.rasterize_layers_backward_cuda(frame_layers, verts, faces, _cu(s["ray_o"]), _cu(s["ray_d"]), fb, ft))
        assert np.isfinite(got).all() and np.abs(want).max() > 0
        print(name, L, g_b is None, g_t is None, rel_linf(got, want), rel_linf(got, full))
        assert rel_linf(got, want) <= GRAD_TOL and rel_linf(got, full) <= GRAD_TOL, (name, L)
    if L == 17 and name == "soup":
        assert int(cnt.max()) > 16


# ---- the backward tables' overflow route at an offset ------------------------------------------------------------------------------
def test_backward_table_overflow_in_a_window():
    """One crowded window (layer_composite_ref's crowded ortho scene, 64 x 48, unaligned origins): every 16 x 16 WINDOW tile
    lists more distinct faces than the face table holds, so k_rasterize_bwd takes its overflow route with an origin.
    k_coverage_bwd's table holds only faces with a non-zero Jacobian, and the crowded scene's faces cover every pixel of the
    frame fully (none is partial: nothing would enter the table), so its overflow route runs on coverage_ref.overflow_case --
    one tile of 1024 small triangles -- moved to an unaligned origin of a larger frame."""
    sc, kind = lref.crowded_case("overflow_L4")
    H, W = sc["render_layers"].shape[1:3]
    pm, pw, ph = np.array([[9, 5], [20, 11]], np.int32), 40, 33
    F = sc["faces"].shape[0]
    rl = wref.cut(sc["render_layers"], pm, pw, ph)
    lo, hi = lref.distinct_blended_per_tile(dict(blend=(rl >= 0) & (rl < F), fs=rl))
    full_tiles = [len(np.unique(rl[b, y:y + 16, x:x + 16])) for b in range(2) for y in (0, 16) for x in (0, 16)]
    print(f"crowded window: {lo}..{hi} distinct listed faces per window tile ({min(full_tiles)} at least in the full tiles), "
          f"table of {table_capacity()} slots")
    assert min(full_tiles) > table_capacity()
    ro, rd = wref.cut(sc["ray_o"], pm, pw, ph), wref.cut(sc["ray_d"], pm, pw, ph)
    gen = torch.Generator().manual_seed(10)
    gb, gt = torch.randn(rl.shape + (3,), generator=gen), torch.randn(rl.shape, generator=gen)
    with _C.window(_cu(pm), W, H):
        got = _np(_C.rasterize_layers_backward_cuda(_cu(rl), _cu(sc["verts"]), _cu(sc["faces"]), _cu(ro), _cu(rd), gb.cuda(), gt.cuda()))
    want = rref.grads64(sc["verts"], sc["faces"], rl, ro, rd, gb, gt)
    assert np.isfinite(got).all() and np.abs(want).max() > 0
    assert rel_linf(got, want) <= GRAD_TOL, rel_linf(got, want)
    # k_coverage_bwd: the one-tile case at origin (21, 6) of a 48 x 32 frame
    c = cref.overflow_case()
    org = np.array([[21, 6]], np.int32)
    vi = (c["verts_image"] + org[0].astype(f32)).astype(f32)
    frame_layers, frame_g = wref.embed(c["render_layers"], org, 48, 32, -1), wref.embed(c["g"], org, 48, 32, 0)
    info = cref.coverage32(frame_layers, vi, c["faces"], 1.0)
    live = wref.cut((np.abs(info["J"]).max((-1, -2)) > 0), org, 16, 16)
    n_live = len(np.unique(c["render_layers"][live]))
    print(f"coverage overflow window: {n_live} faces with a Jacobian in the tile, table of {table_capacity()} slots")
    assert n_live > table_capacity()
    want = cref.grad_image64(frame_layers, vi, c["faces"], 1.0, frame_g, info)
    with _C.window(_cu(org), 48, 32):
        got = _np(_C.coverage_backward_cuda(_cu(c["render_layers"]), _cu(vi), _cu(c["faces"]), 1.0, _cu(c["g"])))
        cov = _C.coverage_cuda(_cu(c["render_layers"]), _cu(vi), _cu(c["faces"]), 1.0)
    _same(cov, wref.cut(info["cov"], org, 16, 16), "overflow window forward")
    assert not got[want == 0].any() and rel_linf(got, want) <= GRAD_TOL, rel_linf(got, want)


# ---- the pipeline --------------------------------------------------------------------------------------------------------------
def test_pipeline_on_a_window():
    """rasterize -> interpolate -> texture -> coverage -> composite on window (c) of a lattice: the forward equals, bit for bit,
    the crop of the same pipeline on the full frame at every pixel whose ids agree (counted: here all of them), and
    loss.backward() reaches verts, the UV table, the texture and the opacities.  A thread other than the forward's runs the
    backward (autograd's own), so the origins travel with the graph."""
    W, H, bidx, L, T = 72, 56, [1, 0], 3, 0.75
    ts = scenes.tet_lattice(W, H, 4, seed=scenes.SEED_BASE + 81, num_cams=2).to("cuda")
    r = dm2.Renderer(ts.mv, ts.proj, W, H, "cuda")
    pm, pw, ph = wref.windows(W, H)["c"]
    gen = torch.Generator().manual_seed(41)
    Pn, F = ts.verts.shape[0], ts.faces.shape[0]
    uv0 = torch.rand((Pn, 2), generator=gen).cuda()
    tex0 = torch.rand((16, 12, 3), generator=gen).cuda()
    op0 = (torch.rand(F, generator=gen) * 0.85 + 0.05).cuda()
    bg = torch.tensor([0.2, 0.5, 0.9]).cuda()

    def run(window):
        kw = dict(patch_min=_cu(pm), patch_width=pw, patch_height=ph) if window else {}
        leaves = [x.clone().requires_grad_(True) for x in (ts.verts, uv0, tex0, op0)]
        verts, uvt, tex, op = leaves
        layers, cnt, bary, t = r.rasterize(bidx, verts, ts.faces, L, **kw)
        uv = r.interpolate(layers, bary, uvt, ts.faces)
        values = r.texture(uv, tex, layers)
        cov = r.coverage(bidx, layers, verts, ts.faces, temperature=T, **({"patch_min": kw["patch_min"]} if window else {}))
        out, acc = r.composite(values, op[layers.clamp(min=0).long()] * cov, layers, bg)
        return leaves, layers, (uv, values, cov, out, acc)

    lw, ids_w, outs_w = run(True)
    lf, ids_f, outs_f = run(False)
    ids_crop = wref.cut(_np(ids_f), pm, pw, ph)
    agree = (_np(ids_w) == ids_crop).all(-1)
    print(f"pipeline: ids agree at {int(agree.sum())} of {agree.size} window pixels")
    assert agree.mean() > 0.99 and (ids_crop >= 0).any(-1).mean() > 0.3
    for k, (a, b) in enumerate(zip(outs_w, outs_f)):
        a, b = _np(a), wref.cut(_np(b), pm, pw, ph)
        assert a.shape == b.shape
        assert np.array_equal(_bits(a)[agree], _bits(b)[agree]), k
    out, acc = outs_w[3], outs_w[4]
    wo, wa = torch.randn(out.shape, generator=gen).cuda(), torch.randn(acc.shape, generator=gen).cuda()
    loss = (out * wo).sum() + (acc * wa).sum()
    import threading
    th = threading.Thread(target=loss.backward)
    th.start(); th.join()
    # the full frame with the upstream gradients embedded in zeros: the same gradients
    fo, fa = outs_f[3], outs_f[4]
    ((fo * _cu(wref.embed(_np(wo), pm, W, H, 0))).sum() + (fa * _cu(wref.embed(_np(wa), pm, W, H, 0))).sum()).backward()
    for name, a, b in zip(("verts", "uv table", "texture", "opacities"), lw, lf):
        assert a.grad is not None and torch.isfinite(a.grad).all() and float(a.grad.abs().max()) > 0, name
        if agree.all():
            e = rel_linf(_np(a.grad), _np(b.grad))
            print("pipeline grad", name, e)
            assert e <= 1e-3, (name, e)            # (test_gpu_coverage_op.py's MODULE_TOL: two fp32 atomic orders of one sum)


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_window_argument_checks():
    ts, scd, lr = _module_scene(False)
    W, H, L = ts.width, ts.height, 2
    m = {k: _cu(a) for k, a in _material(ts.verts.shape[0], ts.faces.shape[0]).items()}
    pm = lambda *rows: torch.tensor(rows, dtype=torch.int32).cuda()
    gen_args = ([1, 0], scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, scd.faces_existence, L)
    layers = torch.full((2, 20, 30, L), -1, dtype=torch.int32).cuda()
    ren = lambda p: lr.render([1, 0], layers, scd.verts, scd.faces, m["verts_color"], m["faces_opacity"], m["faces_intense"],
                              m["background"], patch_min=p)
    calls = {
        "rasterize": lambda p, w, h: lr.rasterize([1, 0], scd.verts, scd.faces, L, patch_min=p, patch_width=w, patch_height=h),
        "generate": lambda p, w, h: lr.generate(*gen_args, patch_min=p, patch_width=w, patch_height=h),
    }
    for what, call in calls.items():
        # a window past the frame: select_rays' two messages
        with pytest.raises(AssertionError, match="Some b_patch_max_x exceed self.width"):
            call(pm([0, 0], [W - 29, 0]), 30, 20)
        with pytest.raises(AssertionError, match="Some b_patch_max_y exceed self.height"):
            call(pm([0, H - 19], [0, 0]), 30, 20)
        with pytest.raises(ValueError, match="must not be negative"):
            call(pm([0, 0], [-1, 3]), 30, 20)
        with pytest.raises(ValueError, match="needs patch_width and patch_height"):
            call(pm([0, 0], [0, 0]), None, None)
        with pytest.raises(ValueError, match="needs patch_width and patch_height"):
            call(pm([0, 0], [0, 0]), 30, None)
        with pytest.raises(ValueError, match="need patch_min"):
            call(None, 30, 20)
        with pytest.raises(ValueError, match=r"patch_min must have dimensions \(2, 2\)"):
            call(pm([0, 0]), 30, 20)
    # coverage and render take the size from render_layers: one that does not fit the origin
    for call in (lambda p: lr.coverage([1, 0], layers, scd.verts, scd.faces, patch_min=p), ren):
        with pytest.raises(AssertionError, match="Some b_patch_max_x exceed self.width"):
            call(pm([W - 29, 0], [0, 0]))
        with pytest.raises(AssertionError, match="Some b_patch_max_y exceed self.height"):
            call(pm([0, 0], [0, H - 19]))
        with pytest.raises(ValueError, match="must not be negative"):
            call(pm([0, -2], [0, 0]))
    # the origins are read back once per call
    reads = []
    real = torch.Tensor.tolist
    torch.Tensor.tolist = lambda self: reads.append(1) or real(self)
    try:
        calls["rasterize"](pm([3, 4], [5, 6]), 30, 20)
        assert len(reads) == 1, len(reads)
    finally:
        torch.Tensor.tolist = real
    # the shim refuses origins it cannot hand to the kernels
    s = wref.scene2("aligned")
    with pytest.raises(RuntimeError, match="patch_min must be int32"):
        with _C.window(torch.zeros((2, 2), dtype=torch.int64).cuda(), W, H):
            _C.coverage_cuda(layers, _cu(s["verts_image"]), _cu(s["faces"]), 1.0)
    with pytest.raises(RuntimeError, match="does not fit"):
        with _C.window(pm([0, 0], [0, 0]), 29, H):
            _C.coverage_cuda(layers, _cu(s["verts_image"]), _cu(s["faces"]), 1.0)
