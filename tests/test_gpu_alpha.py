"""The alpha (coverage) image: Renderer.forward(..., return_alpha=True), LayeredRenderer.render(..., return_alpha=True), and
the C entry points under them (dm2_forward_alpha, dm2_backward's and dm2_layers_composite_backward's dL_dout_alpha).

The reference for all of it is an ordinary colour render.  With verts_color[:, 2] = 0 and background[2] = -1 the blue channel
is 0 + T * (-1), so 1 + color[..., 2] is 1 - T bit for bit, and the gradients of <g_A, alpha> are the colour op's gradients
for dL/dcolor = (0, 0, g_A), dL/ddepth = 0 on that scene -- all but verts_color, which alpha does not touch.  The CPU oracle,
the layered restatement (tests/layer_composite_ref.py) and the two-output GPU op serve as references unchanged."""
import contextlib

import numpy as np
import pytest
import torch

import layer_composite_ref as lref
from util import GRAD_NAMES, GRAD_TOL, capture_forward_args, rel_linf, scatter_aa_grad_to_verts, scenes, soup_args, \
    to_numpy_args

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu


def _orc():
    from oracle import cpu as orc
    return orc


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.int32)


def _dev(args):
    return [a.cuda() if torch.is_tensor(a) else a for a in args]


def zero_channel(args):
    """The 21 arguments with verts_color[:, 2] = 0 and background[2] = -1: blue = -T."""
    a = list(args)
    vc = a[6].clone(); vc[:, 2] = 0.0; a[6] = vc
    bg = a[0].clone(); bg[2] = -1.0; a[0] = bg
    return a


def _soup(W, H, F, seed, temp, dc=4.0):
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + seed, depth_complexity=dc)
    return capture_forward_args(sc, [0], [[0, 0]], W, H, temp, 20)[0]


@contextlib.contextmanager
def _flags(f):
    old = _C.set_flags(f)
    try:
        yield
    finally:
        _C.set_flags(old)


def _bwd(out, dargs, gc, gd, bin_buf=None, **kw):
    return _C.render_backward_cuda(out[0], *dargs, gc, gd, out[7], out[8] if bin_buf is None else bin_buf, out[9], out[3], out[4],
                                   out[5], out[6], **kw)


def _check_alpha_forward(alpha, ref_T, zref_color):
    a = alpha.cpu().numpy()
    assert a.dtype == np.float32
    want = np.float32(1.0) - ref_T.reshape(a.shape)
    assert np.array_equal(_bits(a), _bits(want)), int((_bits(a) != _bits(want)).sum())
    assert np.array_equal(_bits(a), _bits(np.float32(1.0) + zref_color[..., 2]))


# ---- 1. forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [1.0, 0.0])
@pytest.mark.parametrize("kernels", ["default", "legacy"])
def test_forward_alpha_bit_exact(temp, kernels):
    """B = 2 patches at offsets: alpha bit-equal to 1 - final_T of the oracle and to 1 + blue of the zero-channel render;
    colour and depth bit-equal to the two-output forward; the same under torch.no_grad() (DM2_FLAG_NO_BACKWARD)."""
    orc = _orc()
    args, _ = soup_args(160, 112, 700, scenes.SEED_BASE + 81, temp=temp, cams=2, batch_idx=(1, 0),
                        patch_min=[[16, 8], [40, 32]], pw=96, ph=64)
    ref = orc.render_forward_cuda(*to_numpy_args(args))
    zref = orc.render_forward_cuda(*to_numpy_args(zero_channel(args)))
    assert np.array_equal(_bits(ref.final_T), _bits(zref.final_T))
    dargs = _dev(args)
    flags = _C.DM2_FLAG_LEGACY_KERNELS if kernels == "legacy" else 0
    with _flags(flags):
        plain = _C.render_forward_cuda(*dargs)
        with _C.alpha_output(True):
            out = _C.render_forward_cuda(*dargs)
        assert len(plain) == 10 and len(out) == 11
        with torch.no_grad(), _C.alpha_output(True):
            leaves = [a.clone().requires_grad_(True) if i in (4, 6, 7) else a for i, a in enumerate(dargs)]
            c_ng, d_ng, a_ng = dm2.RenderFunction.apply(*leaves)
    torch.cuda.synchronize()
    alpha = out[10]
    assert alpha.shape == (2, 64, 96)
    _check_alpha_forward(alpha, ref.final_T, zref.color)
    _check_alpha_forward(a_ng, ref.final_T, zref.color)
    for i in (1, 2):
        assert torch.equal(out[i], plain[i])
    assert np.array_equal(_bits(out[1].cpu().numpy()), _bits(ref.color))
    assert np.array_equal(_bits(c_ng.cpu().numpy()), _bits(ref.color)) and np.array_equal(_bits(d_ng.cpu().numpy()), _bits(ref.depth))
    a = alpha.cpu().numpy()
    assert (a == 0).any() and (a > 0).any()
    assert not a.reshape(-1)[ref.n_contrib.reshape(-1) == 0].any()                     # no contributor: alpha is 0


def test_forward_alpha_empty_scene():
    """Nothing rendered (F == 0, the early-out of render_forward_cuda): alpha is zeros; and a backward of it is zeros."""
    args = list(_soup(64, 48, 50, 82, 1.0))
    F0 = 0
    args[5] = args[5][:F0]; args[7] = args[7][:F0]; args[10] = args[10][:, :F0]
    for k in range(12, 17):
        args[k] = args[k][:, :F0]
    args[17] = args[17][:, :F0]
    dargs = _dev(args)
    with _C.alpha_output(True):
        out = _C.render_forward_cuda(*dargs)
    assert out[0] == 0 and out[10].shape == (1, 48, 64) and out[10].dtype == torch.float32
    assert not out[10].any()
    gA = torch.ones((1, 48, 64), device="cuda")
    g = _bwd(out, dargs, torch.zeros((1, 48, 64, 3), device="cuda"), torch.zeros((1, 48, 64), device="cuda"), dL_dout_alpha=gA)
    assert all(not x.any() for x in g)


# ---- 2, 4. gradients of <g_A, alpha> on every backward route ----------------------------------------------------------------
ROUTES = ["pool", "masks_only", "point", "unknown_with_pool", "unknown_masks_only", "unknown_point", "legacy"]


def _alpha_route(route, to_verts, edge=False):
    orc = _orc()
    temp = 0.0 if "point" in route else 1.0
    args = list(_soup(96, 64, 500, 64 if not edge else 83, temp, dc=4.0 if not edge else 9.0))
    if edge:
        # opacity exactly 1.0 on every third face (the alpha_is_one branch), 0.95 elsewhere: many pixels stop at T < T_EPS
        op = torch.full_like(args[7], 0.95); op[::3] = 1.0; args[7] = op
    zargs = zero_channel(args)
    ref = orc.render_forward_cuda(*to_numpy_args(zargs))
    B, H, W = ref.depth.shape
    rng = np.random.default_rng(11)
    gA = rng.standard_normal((B, H, W)).astype(np.float32)
    gc = np.zeros((B, H, W, 3), np.float32); gc[..., 2] = gA
    gref = orc.render_backward_cuda(ref, gc, np.zeros((B, H, W), np.float32))
    dargs = _dev(args)
    flags = _C.DM2_FLAG_LEGACY_KERNELS if route == "legacy" else 0
    budget = _C._pool_budget
    try:
        if "masks_only" in route:
            _C._pool_budget = lambda N, R: 0
        with _flags(flags), _C.alpha_output(True), _C.aa_grad_to_verts(to_verts):
            out = _C.render_forward_cuda(*dargs)
    finally:
        _C._pool_budget = budget
    want_mode = {"legacy": _C.FWD_NONE}.get(route, _C.FWD_POINT if "point" in route else _C.FWD_MASKS if "masks_only" in route
                                          else _C.FWD_POOL)
    assert _C.last_forward_mode() == want_mode
    _check_alpha_forward(out[10], ref.final_T, ref.color)
    if edge:
        assert (ref.final_T < 1e-4).sum() > 100
        if temp == 0.0:
            assert (ref.final_T == 0).any()
    bin_buf = out[8].clone() if route.startswith("unknown") else None         # (the shim's note of the mode is gone)
    zc, zd = torch.zeros((B, H, W, 3), device="cuda"), torch.zeros((B, H, W), device="cuda")
    with _flags(flags), _C.aa_grad_to_verts(to_verts):
        for _ in range(2):                                                     # (a second backward of the same forward)
            g = [x.cpu().numpy() for x in _bwd(out, dargs, zc, zd, bin_buf, dL_dout_alpha=torch.from_numpy(gA).cuda())]
            for name in ("verts_color", "verts_ndc", "faces_intense"):
                assert not g[GRAD_NAMES.index(name)].any(), name
            assert rel_linf(g[0], gref["verts"]) <= GRAD_TOL
            assert rel_linf(g[2], gref["faces_opacity"]) <= GRAD_TOL, rel_linf(g[2], gref["faces_opacity"])
            assert np.abs(g[2]).max() > 0
            if to_verts:
                na = to_numpy_args(zargs)
                want = scatter_aa_grad_to_verts(gref["aa_face_verts"], na[12], na[9], na[5])
                assert g[5].shape == want.shape
            else:
                want = gref["aa_face_verts"]
            assert rel_linf(g[5], want) <= GRAD_TOL, rel_linf(g[5], want)
            assert (temp == 0.0) == (not np.abs(g[5]).any())


@pytest.mark.parametrize("to_verts", [False, True], ids=["aa_tables", "aa_to_verts"])
@pytest.mark.parametrize("route", ROUTES)
def test_alpha_gradients_every_route(route, to_verts):
    _alpha_route(route, to_verts)


@pytest.mark.parametrize("route", ["pool", "masks_only", "point", "legacy"])
def test_alpha_gradients_opaque_faces_and_early_stop(route):
    _alpha_route(route, False, edge=True)


# ---- 3. colour, depth and alpha together --------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [1.0, 0.0])
def test_color_depth_alpha_together(temp):
    orc = _orc()
    args = _soup(96, 64, 500, 84, temp)
    ref = orc.render_forward_cuda(*to_numpy_args(args))
    zref = orc.render_forward_cuda(*to_numpy_args(zero_channel(args)))
    B, H, W = ref.depth.shape
    rng = np.random.default_rng(12)
    gc = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    gd = rng.standard_normal((B, H, W)).astype(np.float32)
    gA = rng.standard_normal((B, H, W)).astype(np.float32)
    g1 = orc.render_backward_cuda(ref, gc, gd)
    gcz = np.zeros_like(gc); gcz[..., 2] = gA
    g2 = orc.render_backward_cuda(zref, gcz, np.zeros_like(gd))
    dargs = _dev(args)
    with _C.alpha_output(True):
        out = _C.render_forward_cuda(*dargs)
    g = [x.cpu().numpy() for x in _bwd(out, dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(),
                                       dL_dout_alpha=torch.from_numpy(gA).cuda())]
    for name, x in zip(GRAD_NAMES, g):
        want = g1[name] if name == "verts_color" else g1[name].astype(np.float64) + g2[name]
        assert np.abs(x - want).max() <= 1e-5 * max(np.abs(want).max(), 1e-12), name


# ---- 5, 6. the module path ----------------------------------------------------------------------------------------------------
def _module_grads(r, sc, loss_fn, return_alpha, temp=1.0):
    leaves = [sc.verts.clone().requires_grad_(True), sc.verts_color.clone().requires_grad_(True),
              sc.faces_opacity.clone().requires_grad_(True), sc.faces_intense.clone().requires_grad_(True)]
    out = r([0], torch.zeros((1, 2), dtype=torch.int64, device="cuda"), r.width, r.height, leaves[0], sc.faces, leaves[1],
            leaves[2], leaves[3], sc.background, aa_temperature=temp, return_alpha=return_alpha)
    loss_fn(out).backward()
    torch.cuda.synchronize()
    return out, [x.grad for x in leaves]


PREPS = [dict(fused_prep=False), dict(fused_prep=True, tables_from_image=False), dict(fused_prep=True, tables_from_image=True),
         dict(fused_prep=True, tables_from_image=True, analytic_rays=True), dict(fused_prep=False, analytic_rays=True)]


@pytest.mark.parametrize("prep", range(len(PREPS)))
def test_module_alpha_gradients(prep):
    W, H = 96, 64
    sc = scenes.triangle_soup(W, H, 500, scenes.SEED_BASE + 85, shared_verts=True).to("cuda")
    r = dm2.Renderer(sc.mv, sc.proj, W, H, "cuda", **PREPS[prep])
    gA = torch.randn((1, H, W), generator=torch.Generator().manual_seed(13)).cuda()
    out, ga = _module_grads(r, sc, lambda o: (gA * o[2]).sum(), True)
    assert len(out) == 3 and out[2].shape == (1, H, W)
    zsc = scenes.triangle_soup(W, H, 500, scenes.SEED_BASE + 85, shared_verts=True).to("cuda")
    zsc.verts_color = zsc.verts_color.clone(); zsc.verts_color[:, 2] = 0.0
    zsc.background = zsc.background.clone(); zsc.background[2] = -1.0
    zout, gz = _module_grads(r, zsc, lambda o: (gA * o[0][..., 2]).sum(), False)
    assert torch.equal(out[2], 1.0 + zout[0][..., 2])
    assert ga[1] is None or not ga[1].any()                              # verts_color
    assert ga[3] is None or not ga[3].any()                              # faces_intense
    for i in (0, 2):                                                     # verts, faces_opacity
        assert ga[i].abs().max() > 0
        assert rel_linf(ga[i].cpu().numpy(), gz[i].cpu().numpy()) <= 1e-5, (i, rel_linf(ga[i].cpu().numpy(), gz[i].cpu().numpy()))


@pytest.mark.parametrize("temp", [1.0, 0.0])
def test_unused_alpha_costs_nothing(temp):
    """An alpha returned but left out of the loss: the backward is the two-output op's call (no alpha gradient reaches the
    library; same upstream gradients), and the gradients agree with return_alpha=False."""
    W, H = 96, 64
    sc = scenes.triangle_soup(W, H, 500, scenes.SEED_BASE + 86, shared_verts=True).to("cuda")
    r = dm2.Renderer(sc.mv, sc.proj, W, H, "cuda")
    g = torch.Generator().manual_seed(14)
    wc, wd = torch.randn((1, H, W, 3), generator=g).cuda(), torch.randn((1, H, W), generator=g).cuda()
    calls = []
    real = _C.render_backward_cuda

    def spy(*a, **kw):
        calls.append((kw, a[22].clone(), a[23].clone()))
        return real(*a, **kw)
    _C.render_backward_cuda = spy
    try:
        res = [_module_grads(r, sc, lambda o: (o[0] * wc).sum() + (o[1] * wd).sum(), ra, temp) for ra in (False, True)]
    finally:
        _C.render_backward_cuda = real
    (o0, g0), (o1, g1) = res
    assert len(o1) == 3 and torch.equal(o0[0], o1[0]) and torch.equal(o0[1], o1[1])
    assert calls[0][0] == {} and calls[1][0] == {}
    assert torch.equal(calls[0][1], calls[1][1]) and torch.equal(calls[0][2], calls[1][2])
    for a, b in zip(g0, g1):
        assert rel_linf(b.cpu().numpy(), a.cpu().numpy()) <= 1e-6


# ---- 7. the layered path --------------------------------------------------------------------------------------------------------
def _layer_args(inp):
    t = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).cuda() for k, v in inp.items()}
    return [t[k] for k in ("render_layers", "verts", "faces", "verts_color", "faces_opacity", "faces_intense", "verts_ndc",
                           "background", "ray_o", "ray_d")]


def _check_layered(inp, seed):
    args = _layer_args(inp)
    leaves = [a.clone().requires_grad_(True) if i in (3, 4, 5, 6) else a for i, a in enumerate(args)]
    with _C.alpha_output(True):
        color, depth, alpha = dm2.LayeredCompositeFunction.apply(*leaves)
    fwd = lref.forward32(*[a.cpu() for a in args])
    assert np.array_equal(_bits(alpha.detach().cpu().numpy()), _bits(np.float32(1.0) - fwd["final_T"]))
    gA = torch.randn(alpha.shape, generator=torch.Generator().manual_seed(seed)).cuda()
    (gA * alpha).sum().backward()
    torch.cuda.synchronize()
    zargs = [a.cpu() for a in args]
    zargs[3] = zargs[3].clone(); zargs[3][:, 2] = 0.0
    zargs[7] = zargs[7].clone(); zargs[7][2] = -1.0
    zfwd = lref.forward32(*zargs)
    assert np.array_equal(_bits(alpha.detach().cpu().numpy()), _bits(np.float32(1.0) + zfwd["color"][..., 2]))
    gcz = torch.zeros(color.shape, dtype=torch.float64); gcz[..., 2] = gA.cpu().double()
    want = lref.grads64(zfwd, zargs[2], zargs[3], zargs[4], zargs[5], zargs[6], zargs[7], gcz,
                        torch.zeros(depth.shape, dtype=torch.float64))
    got = dict(verts_color=leaves[3].grad, faces_opacity=leaves[4].grad, faces_intense=leaves[5].grad, verts_ndc=leaves[6].grad)
    for name in ("verts_color", "faces_intense", "verts_ndc"):
        assert got[name] is None or not got[name].any(), name
    g = got["faces_opacity"].cpu().numpy()
    assert np.abs(g).max() > 0
    assert rel_linf(g, want["faces_opacity"]) <= GRAD_TOL, rel_linf(g, want["faces_opacity"])
    return fwd


@pytest.mark.parametrize("L", [5, 12])
def test_layered_alpha_hand_built_lists(L):
    """Holes, out-of-range ids, repeats, opacities of exactly 0 and 1; L = 12 takes the chunked backward."""
    sc = lref.ortho_scene(B=2, H=37, W=45, L=L, F=11, seed=L + 40)
    rl = sc["render_layers"]
    rl[:, ::3, :, 1] = rl[:, ::3, :, 0]
    sc["faces_opacity"][[2, 5]] = [0.0, 1.0]
    fwd = _check_layered(sc, seed=L)
    assert fwd["blend"].sum() > 100


@pytest.mark.parametrize("name", list(lref.CROWDED))
def test_layered_alpha_table_overflow_route(name):
    """k_layer_composite_bwd<true> where the face table overflows or is nearly full (test_gpu_layer_composite.py's crowded
    scenes): the alpha term goes straight to global memory in g[LC_OP]."""
    from test_gpu_layer_composite import crowded
    fwd = _check_layered(crowded(name, "alpha"), seed=21)
    assert fwd["blend"].sum() > 20000 and (fwd["final_T"] == 0.0).any()


@pytest.mark.parametrize("name", list(lref.CROWDED))
def test_layered_color_depth_alpha_together_table_overflow_route(name):
    """Colour, depth and alpha in one loss on the crowded scenes, so that the alpha term and the colour terms share an
    overflowing g[LC_OP].  The zero-channel scene is the reference: its blue channel is -T, alpha = 1 + blue, so with the
    upstream colour gradient on channels 0 and 1 only the loss is the restatement's for dL/dcolor = (g_0, g_1, g_A).  All four
    gradients against lref.grads64 of that scene; of verts_color the channels 0 and 1 (alpha does not reach the colours: the
    kernel's blue column is 0, the restatement's is the blue channel's own)."""
    from test_gpu_layer_composite import crowded
    sc = crowded(name, "colour + depth + alpha")
    sc["verts_color"][:, 2] = 0.0
    sc["background"][2] = -1.0
    args = _layer_args(sc)
    leaves = [a.clone().requires_grad_(True) if i in (3, 4, 5, 6) else a for i, a in enumerate(args)]
    with _C.alpha_output(True):
        color, depth, alpha = dm2.LayeredCompositeFunction.apply(*leaves)
    fwd = lref.forward32(*[a.cpu() for a in args])
    for got, want in ((color, fwd["color"]), (depth, fwd["depth_raw"]), (alpha, np.float32(1.0) - fwd["final_T"]),
                      (alpha, np.float32(1.0) + fwd["color"][..., 2])):
        assert np.array_equal(_bits(got.detach().cpu().numpy()), _bits(want))
    gen = torch.Generator().manual_seed(22)
    gc = torch.randn(color.shape, generator=gen); gc[..., 2] = 0.0
    gd = torch.randn(depth.shape, generator=gen)
    gA = torch.randn(alpha.shape, generator=gen)
    ((gc.cuda() * color).sum() + (gd.cuda() * depth).sum() + (gA.cuda() * alpha).sum()).backward()
    torch.cuda.synchronize()
    gcz = gc.double().clone(); gcz[..., 2] = gA.double()
    cargs = [a.cpu() for a in args]
    want = lref.grads64(fwd, cargs[2], cargs[3], cargs[4], cargs[5], cargs[6], cargs[7], gcz, gd.double())
    got = dict(verts_color=leaves[3].grad, faces_opacity=leaves[4].grad, faces_intense=leaves[5].grad, verts_ndc=leaves[6].grad)
    got = {k: x.cpu().numpy() for k, x in got.items()}
    assert not got["verts_color"][:, 2].any()
    for name_, g, w in (("verts_color", got["verts_color"][:, :2], want["verts_color"][:, :2]),
                        ("faces_opacity", got["faces_opacity"], want["faces_opacity"]),
                        ("faces_intense", got["faces_intense"], want["faces_intense"]),
                        ("verts_ndc", got["verts_ndc"], want["verts_ndc"])):
        assert np.isfinite(g).all() and np.abs(w).max() > 0, name_
        assert rel_linf(g, w) <= GRAD_TOL, (name_, rel_linf(g, w))
    # the alpha term is in it: the opacity gradient of the same loss without alpha differs
    no_alpha = lref.grads64(fwd, cargs[2], cargs[3], cargs[4], cargs[5], cargs[6], cargs[7], gc.double(), gd.double())
    assert rel_linf(no_alpha["faces_opacity"], want["faces_opacity"]) > 0.01


def test_layered_alpha_generated_layers():
    W, H, bidx = 128, 96, [1, 0]
    ts = scenes.tet_lattice(W, H, 5, seed=scenes.SEED_BASE + 87, num_cams=2).to("cuda")
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda")
    layers, _ = lr.generate(bidx, ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, 10)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    ndc, _ = lr.compute_verts_ndc_image(ts.verts, ts.mv[bidx], ts.proj[bidx])
    rng = np.random.RandomState(15)
    inp = dict(render_layers=layers, verts=ts.verts, faces=ts.faces, verts_ndc=ndc.contiguous(),
               ray_o=lr.ray_o[bidx].contiguous(), ray_d=lr.ray_d[bidx].contiguous(),
               verts_color=rng.uniform(0, 1, (P, 3)).astype(np.float32), faces_opacity=rng.uniform(0.05, 0.95, F).astype(np.float32),
               faces_intense=rng.uniform(0.5, 1.5, (2, F)).astype(np.float32), background=np.array([0.1, 0.3, 0.7], np.float32))
    fwd = _check_layered(inp, seed=16)
    assert fwd["blend"].sum() > 1000
    # the module: alpha as a third output, unused alpha leaves the gradients of the two-output render
    leaves = [torch.from_numpy(inp[k]).cuda().requires_grad_(True) for k in ("verts_color", "faces_opacity", "faces_intense")]
    g = torch.Generator().manual_seed(17)
    wc, wd = torch.randn((2, H, W, 3), generator=g).cuda(), torch.randn((2, H, W), generator=g).cuda()
    grads, outs = [], []
    for ra in (False, True):
        for x in leaves:
            x.grad = None
        out = lr.render(bidx, layers, ts.verts, ts.faces, *leaves, torch.from_numpy(inp["background"]).cuda(), return_alpha=ra)
        ((out[0] * wc).sum() + (out[1] * wd).sum()).backward()
        outs.append(out)
        grads.append([x.grad.clone() for x in leaves])
    assert len(outs[1]) == 3 and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(_bits(outs[1][2].detach().cpu().numpy()), _bits(np.float32(1.0) - fwd["final_T"]))
    for a, b in zip(*grads):                           # (same kernel and inputs; LDS / global atomics in another order)
        assert rel_linf(b.cpu().numpy(), a.cpu().numpy()) <= 1e-6


def test_layered_alpha_agrees_with_renderer_at_temperature_zero():
    from test_gpu_layer_composite import _material, _sheets
    W, H, S = 96, 80, 5
    mv, proj = scenes.camera(W, H)
    mv, proj = mv[None].cuda(), proj[None].cuda()
    verts, faces = _sheets(W, H, S, 5)
    P, F = verts.shape[0], faces.shape[0]
    mat = _material(P, F, 1, 6)
    mat["faces_opacity"] = np.random.RandomState(1).uniform(0.2, 0.8, F).astype(np.float32)
    r = dm2.Renderer(mv, proj, W, H, "cuda")
    lr = dm2.LayeredRenderer(mv, proj, W, H, "cuda")
    ro, rd = r.ray_o[0].cpu().numpy(), r.ray_d[0].cpu().numpy()
    vn, fn = verts.numpy(), faces.numpy()
    ok, t, u, v = lref.ray_tri32(ro[:, :, None, :], rd[:, :, None, :], vn[fn[:, 0]], vn[fn[:, 1]], vn[fn[:, 2]])
    hit = ok & (lref.clamp_code32(u, v) == 0)
    order = np.argsort(np.where(hit, t, np.inf), axis=-1, kind="stable")[..., :S]
    layers = np.where(np.take_along_axis(hit, order, -1), order, -1).astype(np.int32)[None]
    gA = torch.randn((1, H, W), generator=torch.Generator().manual_seed(18)).cuda()
    res = []
    for kind in ("renderer", "layers"):
        opac = torch.from_numpy(mat["faces_opacity"]).cuda().requires_grad_(True)
        common = (verts.cuda(), faces.cuda(), torch.from_numpy(mat["verts_color"]).cuda(), opac,
                  torch.from_numpy(mat["faces_intense"]).cuda(), torch.from_numpy(mat["background"]).cuda())
        if kind == "renderer":
            out = r([0], torch.zeros((1, 2), dtype=torch.int64, device="cuda"), W, H, *common, aa_temperature=0.0, return_alpha=True)
        else:
            out = lr.render([0], torch.from_numpy(layers).cuda(), *common, return_alpha=True)
        (gA * out[2]).sum().backward()
        torch.cuda.synchronize()
        res.append((out[2].detach().cpu().numpy(), opac.grad.cpu().numpy()))
    (a0, g0), (a1, g1) = res
    assert (a0 > 0).sum() > 500
    assert np.abs(a0 - a1).max() <= 1e-6
    assert np.abs(g0).max() > 0 and rel_linf(g1, g0) <= GRAD_TOL


# ---- 8. full size -----------------------------------------------------------------------------------------------------------------
def test_cfg2_full_frame_alpha():
    """bench cfg 2 (512 x 512, 50 k faces) against the zero-channel oracle: alpha bit-exact, <g_A, alpha> gradients within
    GRAD_TOL; the default route (pair pool)."""
    import sys
    from util import ROOT
    sys.path.insert(0, ROOT)
    import bench
    orc = _orc()
    args, _, _, (W, H, F) = bench.build_inputs("cfg2", torch.device("cuda", 0), 0, 1)
    assert (W, H, F) == (512, 512, 50_000)
    cargs = [a.cpu() if torch.is_tensor(a) else a for a in args]
    zref = orc.render_forward_cuda(*to_numpy_args(zero_channel(cargs)), nthreads=orc.max_threads())
    B = zref.depth.shape[0]
    gA = np.random.default_rng(19).standard_normal((B, H, W)).astype(np.float32)
    gcz = np.zeros((B, H, W, 3), np.float32); gcz[..., 2] = gA
    gref = orc.render_backward_cuda(zref, gcz, np.zeros((B, H, W), np.float32), nthreads=orc.max_threads())
    with _C.alpha_output(True):
        out = _C.render_forward_cuda(*args)
    assert _C.last_forward_mode() == _C.FWD_POOL
    _check_alpha_forward(out[10], zref.final_T, zref.color)
    g = [x.cpu().numpy() for x in _bwd(out, args, torch.zeros((B, H, W, 3), device="cuda"), torch.zeros((B, H, W), device="cuda"),
                                       dL_dout_alpha=torch.from_numpy(gA).cuda())]
    for name in ("verts", "faces_opacity", "aa_face_verts"):
        i = GRAD_NAMES.index(name)
        assert rel_linf(g[i], gref[name]) <= GRAD_TOL, (name, rel_linf(g[i], gref[name]))
