"""Renderer.texture_mipmaps and texture(filter_mode="linear-mipmap-linear") on the GPU against the restatement
(tests/texture_mip_ref.py): the chain and the trilinear forward bit-equal, every gradient within GRAD_TOL of float64; what
needs_input_grad launches; unaligned tensors; argument checks; the module path from rasterize to verts.grad.  Then off the
beaten path: a channel and layer grid, the scatter table's overflow route and its opposite (every lane on a few keys), the
branch points of the level of detail, the addressing's edges at every level, images smaller than a tile, max_mip_level."""
import itertools

import numpy as np
import pytest
import torch

import bary_derivatives_ref as bref
import composite_ref as cref
import interpolate_ref as iref
import rasterize_ref as rref
import texture_mip_ref as mref
import texture_ref as tref
from util import GRAD_TOL, rel_linf, scenes, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

SHAPE = (2, 20, 24, 3)                                   # B, H, W, L: 2880 slots, 12 blocks of the flat kernels, 4 tiles per view
TEXTURES = ((16, 8), (8, 8), (6, 10), (5, 7))            # (Ht, Wt): nlev 4, 4, 2, 1
CS = (1, 3, 4, 8)                                        # 4 and 8: the four-channel reads
MODE = "linear-mipmap-linear"
_INPUTS = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _shifted(a):
    """``a`` on the GPU as a view that starts 4 bytes into its storage: the four-channel reads do not apply."""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = _cu(a).reshape(-1)
    v = buf[1:].view(a.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def inputs(size):
    """(uv, uv_da, render_layers) of texture_mip_ref.case at SHAPE (tests/test_texture_mip_cpu.py asserts what they reach)."""
    if size not in _INPUTS:
        _INPUTS[size] = mref.case(SHAPE, *size, seed=11)
    return _INPUTS[size]


def _renderer():
    mv, proj = scenes.camera(32, 16)
    return dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")


@pytest.mark.parametrize("size", TEXTURES + ((64, 64), (2, 2)))
def test_chain_forward_and_backward(size):
    r = _renderer()
    rng = np.random.default_rng(20 + size[0])
    for C, per_view, mx in itertools.product(CS, (False, True), (None, 1)):
        tex = rng.standard_normal(((2,) if per_view else ()) + size + (C,), dtype=np.float32)
        want = mref.mipmaps(tex, mx)
        t = _cu(tex).requires_grad_(True)
        mip = r.texture_mipmaps(t, mx)
        what = (size, C, per_view, mx)
        assert tuple(mip.shape) == want.shape and mip.dtype == torch.float32, what
        assert np.array_equal(_bits(_np(mip)), _bits(want)), what
        g = rng.standard_normal(want.shape, dtype=np.float32)
        if want.size:
            mip.backward(_cu(g))
            back = mref.mipmaps_backward64(tex.shape, mx, g)
            assert np.abs(back).max() > 0 and rel_linf(_np(t.grad), back) <= GRAD_TOL, what
            again = _C.texture_mipmaps_backward_cuda(t.detach(), mx, _cu(g))
            assert torch.equal(again, t.grad)                                   # a gather: deterministic
        else:
            assert mref.layout(*size, mx)[0] == 1 and (mip.sum() * 1.0).requires_grad
            (mip.sum() * 1.0).backward()
            assert t.grad is not None and not t.grad.any()


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("boundary_mode", mref.BOUNDARIES)
@pytest.mark.parametrize("size", TEXTURES)
def test_sampling_against_restatement(size, boundary_mode, per_view):
    """Forward bit-equal to forward32, dL/dtex, dL/dmip and dL/duv within GRAD_TOL of grads64, for every C, with and without
    render_layers."""
    uv, da, rl = inputs(size)
    rng = np.random.default_rng(30 + size[1])
    big = rng.standard_normal(((2,) if per_view else ()) + size + (max(CS),), dtype=np.float32)
    big[..., 1, 1, :] = -0.0
    for C, layers in itertools.product(CS, (rl, None)):
        tex = np.ascontiguousarray(big[..., :C])
        mip = mref.mipmaps(tex)
        what = (size, boundary_mode, per_view, C, layers is not None)
        args = (_cu(uv), _cu(da), _cu(tex), _cu(mip), _cu(layers), boundary_mode, None)
        out = _np(_C.texture_mip_cuda(*args))
        want = mref.forward32(uv, da, tex, mip, layers, boundary_mode)
        assert out.shape == SHAPE + (C,) and out.dtype == np.float32, what
        assert np.array_equal(_bits(out), _bits(want)), (what, int((_bits(out) != _bits(want)).sum()))
        st = mref.stage(uv, da, *size, layers)
        assert not out[st["empty"]].any() and (np.abs(out[~st["empty"]]).max(-1) > 0).mean() > 0.99, what
        g = rng.standard_normal(SHAPE + (C,), dtype=np.float32)
        dt, dm, du = (_np(x) for x in _C.texture_mip_backward_cuda(*args, _cu(g), True, True, True))
        wt, wm, wu = mref.grads64(uv, da, tex, mip, layers, boundary_mode, None, g)
        assert dt.shape == tex.shape and dm.shape == mip.shape and du.shape == uv.shape, what
        et, em, eu = rel_linf(dt, wt), rel_linf(dm, wm), rel_linf(du, wu)
        print(what, "dtex", et, "dmip", em, "duv", eu)
        assert np.abs(wt).max() > 0 and (not wm.size or np.abs(wm).max() > 0), what
        assert np.isfinite(dt).all() and np.isfinite(dm).all() and np.isfinite(du).all(), what
        assert et <= GRAD_TOL and em <= GRAD_TOL, (what, et, em)
        if size[0] * size[1] > 1:
            assert np.abs(wu).max() > 0, what
        assert eu <= GRAD_TOL, (what, eu)
        assert not du[st["empty"]].any(), what


def test_level_zero_is_the_linear_filter_and_max_mip_level():
    """lod <= 0: the bits of filter_mode="linear"; max_mip_level = 1 against the restatement; a constant texture at every lod."""
    size, C = (16, 8), 3
    uv, da, rl = inputs(size)
    rng = np.random.default_rng(40)
    tex = rng.standard_normal(size + (C,), dtype=np.float32)
    r = _renderer()
    out = _np(r.texture(_cu(uv), _cu(tex), _cu(rl), MODE, "clamp", uv_da=_cu(da)))
    lin = _np(r.texture(_cu(uv), _cu(tex), _cu(rl), "linear", "clamp"))
    st = mref.stage(uv, da, *size, rl)
    low = ~st["empty"] & (st["lod"] <= 0)
    assert low.sum() > 100 and np.array_equal(_bits(out[low]), _bits(lin[low])) and (out[st["two"]] != lin[st["two"]]).any()
    mip1 = mref.mipmaps(tex, 1)
    out1 = _np(r.texture(_cu(uv), _cu(tex), _cu(rl), MODE, "wrap", uv_da=_cu(da), mip=_cu(mip1), max_mip_level=1))
    assert np.array_equal(_bits(out1), _bits(mref.forward32(uv, da, tex, mip1, rl, "wrap", 1)))
    own = _np(r.texture(_cu(uv), _cu(tex), _cu(rl), MODE, "wrap", uv_da=_cu(da), max_mip_level=1))       # the chain built by the call
    assert np.array_equal(_bits(own), _bits(out1))
    flat = np.full(size + (2,), np.float32(0.7))
    outc = _np(r.texture(_cu(uv), _cu(flat), _cu(rl), MODE, uv_da=_cu(da)))
    assert (outc[~st["empty"]] == np.float32(0.7)).all() and not outc[st["empty"]].any()


def test_minified_checkerboard_is_grey():
    """tests/test_texture_mip_cpu.py's input on the GPU: exactly 0.5 from the chain, anything from the bilinear filter."""
    n = 64
    jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    tex = ((ii + jj) % 2).astype(np.float32)[..., None]
    rng = np.random.RandomState(8)
    shape = (1, 16, 16, 1)
    ys, xs = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    step = 8.0 / n
    uv = (np.stack([xs * step, ys * step], -1).reshape(shape + (2,)) + rng.uniform(0, step, shape + (2,))).astype(np.float32)
    da = np.broadcast_to(np.array([step, 0, 0, step], np.float32), shape + (4,)).copy()
    da *= rng.uniform(0.8, 1.25, shape + (1,)).astype(np.float32)
    r = _renderer()
    out = _np(r.texture(_cu(uv), _cu(tex), None, MODE, uv_da=_cu(da)))
    lin = _np(r.texture(_cu(uv), _cu(tex)))
    assert (out == np.float32(0.5)).all() and lin.max() - lin.min() > 0.5


def test_needs_input_grad():
    """Only what needs_input_grad asks for reaches the library: the output pointers of dm2_texture_mip_backward, and no call at
    all when nothing requires grad."""
    size, C = (16, 8), 4
    uv, da, rl = inputs(size)
    rng = np.random.default_rng(41)
    tex = rng.standard_normal(size + (C,), dtype=np.float32)
    mip = mref.mipmaps(tex)
    g = rng.standard_normal(SHAPE + (C,), dtype=np.float32)
    wt, wm, wu = mref.grads64(uv, da, tex, mip, rl, "wrap", None, g)
    r = _renderer()
    lib = _C.load_library()
    real_b, real_m = lib.dm2_texture_mip_backward, lib.dm2_texture_mipmaps_backward
    calls = []

    def spy(*a):
        calls.append(tuple(x.value is not None for x in a[16:19]))               # dL_dtex, dL_dmip, dL_duv
        return real_b(*a)
    lib.dm2_texture_mip_backward = spy
    lib.dm2_texture_mipmaps_backward = lambda *a: calls.append("chain") or real_m(*a)
    try:
        res = {}
        for need in itertools.product((False, True), repeat=3):
            if not any(need):
                continue
            u, t, m = _cu(uv).requires_grad_(need[0]), _cu(tex).requires_grad_(need[1]), _cu(mip).requires_grad_(need[2])
            d = _cu(da).requires_grad_(True)
            out = r.texture(u, t, _cu(rl), MODE, uv_da=d, mip=m)
            out.backward(_cu(g))
            assert calls[-1] == (need[1], need[2], need[0]), (need, calls[-1])
            assert d.grad is None                                                # the level of detail is a constant of the op
            res[need] = tuple(None if x.grad is None else _np(x.grad) for x in (u, t, m))
            for got, want, on in zip(res[need], (wu, wt, wm), need):
                assert (got is None) == (not on) and (got is None or rel_linf(got, want) <= GRAD_TOL), need
        assert len(calls) == 7 and "chain" not in calls
        assert np.array_equal(res[(True, True, True)][0], res[(True, False, False)][0])      # dL/duv: a pure function of the inputs
        # the chain built by the call: the texture's gradient flows through MipmapFunction as well
        del calls[:]
        t = _cu(tex).requires_grad_(True)
        r.texture(_cu(uv), t, _cu(rl), MODE, uv_da=_cu(da)).backward(_cu(g))
        assert calls == [(True, True, False), "chain"]
        assert rel_linf(_np(t.grad), wt + mref.mipmaps_backward64(tex.shape, None, wm)) <= GRAD_TOL
        # nothing requires grad: no graph, no call
        del calls[:]
        out = r.texture(_cu(uv), _cu(tex), _cu(rl), MODE, uv_da=_cu(da), mip=_cu(mip))
        assert out.grad_fn is None
        assert _C.texture_mip_backward_cuda(_cu(uv), _cu(da), _cu(tex), _cu(mip), _cu(rl), "wrap", None, _cu(g), False, False, False) == (None,) * 3
        assert not calls
    finally:
        lib.dm2_texture_mip_backward, lib.dm2_texture_mipmaps_backward = real_b, real_m


@pytest.mark.parametrize("C", [4, 8])
def test_unaligned_tensors_give_the_same_bits(C):
    """tex, mip and the upstream gradient as views that start 4 bytes into their storage: the four-channel reads do not apply;
    the same bits as with aligned tensors."""
    size = (16, 8)
    uv, da, rl = inputs(size)
    rng = np.random.default_rng(42)
    tex = rng.standard_normal((2,) + size + (C,), dtype=np.float32)
    mip = mref.mipmaps(tex)
    g = rng.standard_normal(SHAPE + (C,), dtype=np.float32)
    head, tail = (_cu(uv), _cu(da)), (_cu(rl), "wrap", None)
    out_a = _C.texture_mip_cuda(*head, _cu(tex), _cu(mip), *tail)
    for t, m in ((_shifted(tex), _cu(mip)), (_cu(tex), _shifted(mip)), (_shifted(tex), _shifted(mip))):
        assert torch.equal(_C.texture_mip_cuda(*head, t, m, *tail), out_a)
    assert np.array_equal(_bits(_np(out_a)), _bits(mref.forward32(uv, da, tex, mip, rl, "wrap")))
    ga = _C.texture_mip_backward_cuda(*head, _cu(tex), _cu(mip), *tail, _cu(g), True, True, True)
    gu = _C.texture_mip_backward_cuda(*head, _shifted(tex), _shifted(mip), *tail, _shifted(g), True, True, True)
    assert torch.equal(ga[2], gu[2])
    want = mref.grads64(uv, da, tex, mip, rl, "wrap", None, g)
    for a, u, w in zip(ga, gu, want):
        assert rel_linf(_np(u), w) <= GRAD_TOL and rel_linf(_np(a), w) <= GRAD_TOL


def test_argument_checks():
    size, C = (16, 8), 3
    uv, da, rl = (_cu(x) for x in inputs(size))
    tex = torch.zeros(size + (C,), device="cuda")
    mip = _C.texture_mipmaps_cuda(tex)
    assert tuple(mip.shape) == (42, C)
    ok = _C.texture_mip_cuda(uv, da, tex, mip, rl)
    assert tuple(ok.shape) == SHAPE + (C,)
    for args, name in (((uv[..., :1], da, tex, mip, rl), "uv"), ((uv.double(), da, tex, mip, rl), "uv"),
                       ((uv, da[..., :3], tex, mip, rl), "uv_da"), ((uv, da[:1], tex, mip, rl), "uv_da"), ((uv, da.double(), tex, mip, rl), "uv_da"),
                       ((uv, da, tex[0], mip, rl), "tex"), ((uv, da, tex.half(), mip, rl), "tex"),
                       ((uv, da, tex, mip[:41], rl), "mip"), ((uv, da, tex, mip[:, :2], rl), "mip"), ((uv, da, tex, mip[None], rl), "mip"),
                       ((uv, da, tex, mip.double(), rl), "mip"), ((uv, da, tex, mip, rl[:1]), "render_layers"),
                       ((uv, da, tex, mip, rl.long()), "render_layers")):
        with pytest.raises(RuntimeError, match=name):
            _C.texture_mip_cuda(*args)
    with pytest.raises(RuntimeError, match="mip"):
        _C.texture_mip_cuda(uv, da, tex, mip, rl, "wrap", 1)                   # the whole chain under max_mip_level = 1
    with pytest.raises(RuntimeError, match="mip"):
        _C.texture_mip_cuda(uv, da, tex[None].expand(2, *tex.shape).contiguous(), mip, rl)      # per-view textures, a shared chain
    with pytest.raises(RuntimeError, match="boundary_mode"):
        _C.texture_mip_cuda(uv, da, tex, mip, rl, "mirror")
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.texture_mip_backward_cuda(uv, da, tex, mip, rl, "wrap", None, ok[..., :2], True, True, True)
    with pytest.raises(RuntimeError, match="grad_mip"):
        _C.texture_mipmaps_backward_cuda(tex, None, mip[:41])
    with pytest.raises(RuntimeError, match="tex"):
        _C.texture_mipmaps_cuda(tex[0])
    with pytest.raises(ValueError, match="max_mip_level"):
        _C.texture_mipmaps_cuda(tex, -1)
    for fn, args in ((_C.texture_mip_cuda, (uv.cpu(), da.cpu(), tex.cpu(), mip.cpu(), rl.cpu())), (_C.texture_mip_cuda, (uv, da, tex, mip.cpu(), rl)),
                     (_C.texture_mip_cuda, (uv, da.cpu(), tex, mip, rl)), (_C.texture_mipmaps_cuda, (tex.cpu(),)),
                     (_C.texture_mipmaps_backward_cuda, (tex, None, mip.cpu()))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(*args)
    r = _renderer()
    with pytest.raises(ValueError, match="uv_da"):
        r.texture(uv, tex, rl, MODE)
    with pytest.raises(ValueError, match="uv_da"):
        r.texture(uv, tex, rl, "linear", uv_da=da)
    with pytest.raises(ValueError, match="mip"):
        r.texture(uv, tex, rl, "nearest", mip=mip)
    with pytest.raises(RuntimeError, match="mip"):
        r.texture(uv, tex, rl, MODE, uv_da=da, mip=mip, max_mip_level=2)
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    p = _C._ptr
    B, H, W, L = SHAPE
    assert lib.dm2_texture_mip(B, H, W, L, 16, 8, C, 0, 7, -1, p(rl), p(uv), p(da), p(tex), p(mip), p(ok), None) == 1
    assert lib.dm2_texture_mip(B, H, W, L, 0, 8, C, 0, 0, -1, p(rl), p(uv), p(da), p(tex), p(mip), p(ok), None) == 1
    assert lib.dm2_texture_mip(B, H, W, L, 16, 8, C, 0, 0, -1, p(rl), p(uv), None, p(tex), p(mip), p(ok), None) == 1
    assert lib.dm2_texture_mip(B, H, W, L, 16, 8, C, 0, 0, -1, p(rl), p(uv), p(da), p(tex), None, p(ok), None) == 1
    # 46340^2 texels lie below 2^31 (dm2_texture takes them), with the chain's 23170^2 + ... they do not
    assert lib.dm2_texture_mip(B, H, W, L, 46340, 46340, C, 0, 0, -1, p(rl), p(uv), p(da), p(tex), p(mip), p(ok), None) == 1
    assert lib.dm2_texture_mipmaps(1, 46340, 46340, C, -1, p(tex), p(mip), None) == 1
    assert lib.dm2_texture_mipmaps(1, 16, 8, 0, -1, p(tex), p(mip), None) == 1
    assert lib.dm2_texture_mipmaps(1, 16, 8, C, -1, None, p(mip), None) == 1
    # degenerate sizes: no launch
    launches = []
    real_f = lib.dm2_texture_mip
    lib.dm2_texture_mip = lambda *a: launches.append("f") or real_f(*a)
    try:
        for shape in ((0, 4, 5, 2), (2, 0, 5, 2), (2, 4, 5, 0)):
            e_uv, e_da = torch.zeros(shape + (2,), device="cuda"), torch.zeros(shape + (4,), device="cuda")
            out = _C.texture_mip_cuda(e_uv, e_da, tex, mip, None)
            assert tuple(out.shape) == shape + (C,)
            dt, dm, du = _C.texture_mip_backward_cuda(e_uv, e_da, tex, mip, None, "wrap", None, torch.ones_like(out), True, True, True)
            assert tuple(dt.shape) == tuple(tex.shape) and tuple(dm.shape) == tuple(mip.shape) and tuple(du.shape) == shape + (2,)
        assert not launches
    finally:
        lib.dm2_texture_mip = real_f


def test_module_path_end_to_end():
    """rasterize -> bary_derivatives -> interpolate x 3 -> texture (the chain built by the call) -> composite -> a weighted sum on
    the soup: tex.grad, the UV table's gradient and verts.grad against the same chain put together from the numpy references."""
    s = rref.scene("soup")
    W, H, L, C, size = s["W"], s["H"], 3, 3, (64, 64)
    mv, proj = bref.scene_cameras("soup")
    idx = [0, 1, 2]
    r = dm2.Renderer(_cu(mv), _cu(proj), W, H, "cuda")
    ro, rd = _np(r._camera_rows(r.ray_o, idx)), _np(r._camera_rows(r.ray_d, idx))
    gen = torch.Generator().manual_seed(21)
    faces = _cu(s["faces"])
    F = faces.shape[0]
    uv_faces = torch.arange(3 * F, dtype=torch.int32).reshape(F, 3).cuda()
    # a UV triangle of its own per face, its size 2^-3 .. 2^1.5 of the texture: magnified faces and every level down to 4 x 4
    spread = (2.0 ** (torch.rand((F, 1, 1), generator=gen) * 4.5 - 3.0)).expand(F, 3, 2).reshape(3 * F, 2)
    table0 = (0.5 + (torch.rand((3 * F, 2), generator=gen) - 0.5) * spread).cuda()
    tex0 = torch.randn(size + (C,), generator=gen).cuda()
    alpha = (torch.rand((F,), generator=gen) * 0.8 + 0.1).cuda()
    bg = torch.rand((C,), generator=gen).cuda()
    verts, table, tex = (x.clone().requires_grad_(True) for x in (_cu(s["verts"]), table0, tex0))
    layers, cnt, bary, t = r.rasterize(idx, verts, faces, L)
    dx, dy = r.bary_derivatives(idx, layers, verts, faces)
    uv = r.interpolate(layers, bary, table, uv_faces)
    uv_da = torch.cat([r.interpolate(layers, dx, table, uv_faces), r.interpolate(layers, dy, table, uv_faces)], -1)
    out = r.texture(uv, tex, layers, MODE, uv_da=uv_da)
    img, acc = r.composite(out, alpha, layers, bg)
    wgt = torch.randn(img.shape, generator=gen).cuda()
    (img * wgt).sum().backward()
    for x in (tex.grad, table.grad, verts.grad):
        assert x is not None and torch.isfinite(x).all()
    # the same chain from the references, on the op's own intermediate values
    rl, bn, un, dn = _np(layers), _np(bary), _np(uv), _np(uv_da)
    tn, tabn, ufn = _np(tex0), _np(table0), _np(uv_faces)
    cam = torch.cat((torch.inverse(r.mv[idx]).reshape(-1, 16), torch.inverse(r.proj[idx]).reshape(-1, 16)), dim=1)
    wx, wy = bref.forward32(rl, s["verts"], s["faces"], _np(cam), W, H)
    assert np.array_equal(_bits(_np(dx)), _bits(wx)) and np.array_equal(_bits(_np(dy)), _bits(wy))
    want_da = np.concatenate([iref.forward32(rl, wx, tabn, ufn), iref.forward32(rl, wy, tabn, ufn)], -1)
    assert np.array_equal(_bits(dn), _bits(want_da))
    mip = mref.mipmaps(tn)
    assert np.array_equal(_bits(_np(out)), _bits(mref.forward32(un, dn, tn, mip, rl, "wrap")))
    reach = mref.reach(un, dn, *size, rl)
    print("end to end reaches", reach)
    assert reach["magnified"] > 100 and sum(reach["pairs"]) > 1000
    _, _, n_contrib = cref.forward32(_np(out), _np(alpha), rl, _np(bg))
    dvalues, _ = cref.grads64(_np(out), _np(alpha), rl, _np(bg), n_contrib, _np(wgt), None)
    wt, wm, wu = mref.grads64(un, dn, tn, mip, rl, "wrap", None, dvalues)
    wt = wt + mref.mipmaps_backward64(tn.shape, None, wm)
    wtab, wb = iref.grads64(rl, bn, tabn, ufn, wu)
    wv = rref.grads64(s["verts"], s["faces"], rl, ro, rd, wb, None)
    et, ea, ev = rel_linf(_np(tex.grad), wt), rel_linf(_np(table.grad), wtab), rel_linf(_np(verts.grad), wv)
    print("end to end: tex.grad", et, "uv table grad", ea, "verts.grad", ev)
    assert np.abs(wt).max() > 0 and np.abs(wtab).max() > 0 and np.abs(wv).max() > 0
    assert et <= GRAD_TOL and ea <= GRAD_TOL and ev <= GRAD_TOL


# ---- off the beaten path: the input sets of texture_mip_ref beyond ``case``, each held to its condition by its twin in
# tests/test_texture_mip_cpu.py ----

GRID_CS = (2, 5, 7, 12, 16, 20, 33)                      # CH = 2; a chunk's tail; CV = 3, 4, 5 on the vector path, 33 on the scalar one
GRID_LS = (1, 3, 8)
GRID_TEXTURES = ((16, 8), (32, 32), (6, 10))


def _check(uv, da, tex, mip, rl, boundary_mode, mx, g, what, zero=""):
    """The forward bit-equal to forward32 and, with ``g``, dL/dtex, dL/dmip and dL/duv within GRAD_TOL of grads64 -> (out, (dt, dm,
    du), (wt, wm, wu)).  ``zero``: the gradients ("t", "m", "u") that are all zeros in the reference by construction and must be
    exactly zero; every other is non-zero in the reference."""
    args = (_cu(uv), _cu(da), _cu(tex), _cu(mip), _cu(rl), boundary_mode, mx)
    out = _np(_C.texture_mip_cuda(*args))
    want = mref.forward32(uv, da, tex, mip, rl, boundary_mode, mx)
    assert out.shape == want.shape and out.dtype == np.float32, what
    assert np.array_equal(_bits(out), _bits(want)), (what, int((_bits(out) != _bits(want)).sum()))
    if g is None:
        return out, None, None
    got = tuple(_np(x) for x in _C.texture_mip_backward_cuda(*args, _cu(g), True, True, True))
    ref = mref.grads64(uv, da, tex, mip, rl, boundary_mode, mx, g)
    errs = [rel_linf(a, b) for a, b in zip(got, ref)]
    print(what, "dtex", errs[0], "dmip", errs[1], "duv", errs[2])
    for name, a, b, e in zip("tmu", got, ref, errs):
        assert a.shape == b.shape and np.isfinite(a).all(), (what, name)
        if name in zero or not b.size:
            assert not b.any() and not a.any(), (what, name)
        else:
            assert np.abs(b).max() > 0 and e <= GRAD_TOL, (what, name, e)
    assert not got[2][mref.stage(uv, da, tex.shape[-3], tex.shape[-2], rl, mx)["empty"]].any(), what
    return out, got, ref


def _grid(k):
    return GRID_CS[k // 2], bool(k % 2), GRID_LS[k % 3], GRID_TEXTURES[(k // 3) % 3]


@pytest.mark.parametrize("k", range(2 * len(GRID_CS)))
def test_channel_and_layer_grid(k):
    """A thinned grid, both boundary modes at each point: every C, L, texture size and sharing appears."""
    C, per_view, L, size = _grid(k)
    shape = SHAPE[:3] + (L,)
    uv, da, rl = mref.case(shape, *size, seed=11)
    rng = np.random.default_rng(300 + k)
    tex = rng.standard_normal(((2,) if per_view else ()) + size + (C,), dtype=np.float32)
    mip = mref.mipmaps(tex)
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    for boundary_mode in mref.BOUNDARIES:
        _check(uv, da, tex, mip, rl, boundary_mode, None, g, (k, C, per_view, L, size, boundary_mode))


@pytest.mark.parametrize("C", tref.INST_CS)
def test_every_instantiation_once(C):
    """Both boundary modes x shared and per-view textures at this C on texture_mip_ref.instantiation_case(), with dL/dtex
    alone, dL/dmip alone and both wanted: every instantiation of the sampling kernels that C selects, and both outcomes of the
    scatter's absent-destination skip, at the smallest shape with two views, partial tiles, two layers and empty slots in
    every tile."""
    uv, da, rl = mref.instantiation_case()
    size = mref.INST_TEXTURE
    bad = mref.stage(uv, da, *size, rl)["empty"]
    rng = np.random.default_rng(800 + C)
    g = rng.standard_normal(uv.shape[:4] + (C,), dtype=np.float32)
    for per_view in (False, True):
        tex = rng.standard_normal(((2,) if per_view else ()) + size + (C,), dtype=np.float32)
        mip = mref.mipmaps(tex)
        for boundary_mode in mref.BOUNDARIES:
            what = ("instantiation", C, per_view, boundary_mode)
            out, got, want = _check(uv, da, tex, mip, rl, boundary_mode, None, g, what)
            assert (out[bad] == 0).all(), what
            args = (_cu(uv), _cu(da), _cu(tex), _cu(mip), _cu(rl), boundary_mode, None, _cu(g))
            dt, dm, du = _C.texture_mip_backward_cuda(*args, True, False, False)
            assert dm is None and du is None and rel_linf(_np(dt), want[0]) <= GRAD_TOL, what
            dt, dm, du = _C.texture_mip_backward_cuda(*args, False, True, False)
            assert dt is None and du is None and rel_linf(_np(dm), want[1]) <= GRAD_TOL, what


def test_grid_covers_every_axis():
    seen = [set() for _ in range(4)]
    for k in range(2 * len(GRID_CS)):
        for s, v in zip(seen, _grid(k)):
            s.add(v)
    assert [len(s) for s in seen] == [len(GRID_CS), 2, len(GRID_LS), len(GRID_TEXTURES)]


@pytest.mark.parametrize("boundary_mode", mref.BOUNDARIES)
def test_forward_with_more_channels_than_lanes(boundary_mode):
    """C = 260: 65 groups of four per slot on the vector path, and (unaligned) 260 single channels on the scalar one, more than
    the block has lanes: the sweep's slot stays and its channel moves on by 256."""
    shape, size, C = (1, 4, 5, 2), (16, 8), 260
    uv, da, rl = mref.case(shape, *size, seed=17)
    rng = np.random.default_rng(43)
    tex = rng.standard_normal(size + (C,), dtype=np.float32)
    mip = mref.mipmaps(tex)
    out, _, _ = _check(uv, da, tex, mip, rl, boundary_mode, None, None, ("C = 260", boundary_mode))
    slow = _C.texture_mip_cuda(_cu(uv), _cu(da), _shifted(tex), _shifted(mip), _cu(rl), boundary_mode, None)
    assert np.array_equal(_bits(_np(slow)), _bits(out))


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("C", [3, 16])
def test_table_overflow_route(C, per_view):
    """A 512^2 texture under random uv and footprints of half a texel to eleven: every tile addresses several times the keys the
    scatter's table holds (asserted), in both destination tensors; what finds no slot adds straight to dL/dtex or dL/dmip.
    Asked for alone, each of the two is what it is when both are asked for, up to the order of the atomics."""
    uv, da, rl = mref.overflow_case()
    size, shape = mref.OVERFLOW_SIZE, mref.OVERFLOW_SHAPE
    rng = np.random.default_rng(44 + C)
    tex = rng.standard_normal(((2,) if per_view else ()) + size + (C,), dtype=np.float32)
    mip = mref.mipmaps(tex)
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    for layers, boundary_mode in ((None, "wrap"), (rl, "clamp")):
        least = mref.distinct_keys_per_tile(uv, da, *size, layers, boundary_mode)
        print("distinct keys per tile and layer, at least", least)
        assert least > table_capacity()
        what = ("overflow", C, per_view, layers is not None, boundary_mode)
        _, (dt, dm, du), (wt, wm, wu) = _check(uv, da, tex, mip, layers, boundary_mode, None, g, what)
        args = (_cu(uv), _cu(da), _cu(tex), _cu(mip), _cu(layers), boundary_mode, None, _cu(g))
        t_only = _C.texture_mip_backward_cuda(*args, True, False, False)
        m_only = _C.texture_mip_backward_cuda(*args, False, True, False)
        assert t_only[1] is None and t_only[2] is None and m_only[0] is None and m_only[2] is None
        et, em = rel_linf(_np(t_only[0]), wt), rel_linf(_np(m_only[1]), wm)
        ett, emm = rel_linf(_np(t_only[0]), dt), rel_linf(_np(m_only[1]), dm)
        print(what, "tex alone", et, "against both", ett, "mip alone", em, "against both", emm)
        assert et <= GRAD_TOL and em <= GRAD_TOL and ett <= GRAD_TOL and emm <= GRAD_TOL, (what, et, em, ett, emm)


@pytest.mark.parametrize("C", [1, 3, 16])
def test_magnified_every_lane_on_a_few_keys(C):
    """Every slot magnified into one corner of an (8, 8) texture: at most 16 keys per tile (asserted), all of level 0."""
    uv, da = mref.hot_case_magnified()
    assert 0 < mref.distinct_keys_per_tile(uv, da, 8, 8, worst=max) <= 16
    rng = np.random.default_rng(45)
    for per_view in (False, True):
        tex = rng.standard_normal(((2,) if per_view else ()) + (8, 8, C), dtype=np.float32)
        g = rng.standard_normal(mref.HOT_SHAPE + (C,), dtype=np.float32)
        _check(uv, da, tex, mref.mipmaps(tex), None, "wrap", None, g, ("magnified", C, per_view), zero="m")


@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("size", [(8, 8), (16, 8)])
def test_every_tap_on_the_top_level(size, C):
    """Every slot far beyond the last level (one in eight by r2 = inf): all 28000 slots' taps on the top level's one or two
    texels (asserted), nothing for the texture itself."""
    uv, da = mref.hot_case_beyond(*size)
    st = mref.stage(uv, da, *size)
    assert not st["empty"].any() and not st["two"].any() and (st["j"] == st["nlev"] - 1).all() and (st["lod"] == 64).any()
    rng = np.random.default_rng(46)
    for per_view, boundary_mode in ((False, "wrap"), (True, "clamp")):
        assert mref.distinct_keys_per_tile(uv, da, *size, None, boundary_mode, worst=max) == size[0] // 8
        tex = rng.standard_normal(((2,) if per_view else ()) + size + (C,), dtype=np.float32)
        g = rng.standard_normal(mref.HOT_SHAPE + (C,), dtype=np.float32)
        _, (dt, dm, du), _ = _check(uv, da, tex, mref.mipmaps(tex), None, boundary_mode, None, g, ("beyond", size, C, per_view, boundary_mode),
                                    zero="t" if size == (16, 8) else "tu")       # (one texel: no derivative in uv)
        top = mref.layout(*size)[1][-1][2]
        assert not dm[..., :top, :].any() and dm[..., top:, :].all()


@pytest.mark.parametrize("boundary_mode", mref.BOUNDARIES)
@pytest.mark.parametrize("size,mx", mref.EDGE_TEXTURES)
def test_level_of_detail_edges(size, mx, boundary_mode):
    """texture_mip_ref.lod_edge_footprints: r2 and lod on every branch point and on the floats next to it.  On top of the
    restatement: lod <= 0 gives filter_mode="linear"'s bits; an integer lod between the ends gives the bits of level j alone,
    and the level above receives exactly nothing from those slots."""
    C = 3
    uv, da = mref.lod_edge_case(*size, mx)
    rng = np.random.default_rng(47)
    tex = rng.standard_normal((2,) + size + (C,), dtype=np.float32)
    mip = mref.mipmaps(tex, mx)
    shape = (2,) + mref.EDGE_SHAPE[1:]
    uv, da = np.concatenate([uv, uv]), np.concatenate([da, da])               # (per-view textures: the table under both)
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    what = ("lod edges", size, mx, boundary_mode)
    out, _, _ = _check(uv, da, tex, mip, None, boundary_mode, mx, g, what)
    st = mref.stage(uv, da, *size, None, mx)
    low = st["lod"] <= 0
    lin = _np(_C.texture_cuda(_cu(uv), _cu(tex), None, "linear", boundary_mode))
    assert low.sum() >= 20 and np.array_equal(_bits(out[low]), _bits(lin[low])), what
    _, levels, _ = mref.layout(*size, mx)
    for k in range(1, st["nlev"] - 1):
        whole = st["two"] & (st["f"] == 0) & (st["j"] == k)
        assert whole.sum() >= 4, (what, k)
        alone = tref.forward32(uv, mref.level(tex, mip, k, mx), None, "linear", boundary_mode)
        assert np.array_equal(_bits(out[whole]), _bits(alone[whole])), (what, k)
        gk = np.where(whole[..., None], g, np.float32(0))
        dt, dm, du = (_np(x) for x in _C.texture_mip_backward_cuda(_cu(uv), _cu(da), _cu(tex), _cu(mip), None, boundary_mode, mx, _cu(gk),
                                                                   True, True, True))
        wt, wm, wu = mref.grads64(uv, da, tex, mip, None, boundary_mode, mx, gk)
        h, w, off = levels[k]
        assert np.abs(wm[:, off:off + h * w]).max() > 0 and not wm[:, off + h * w:].any() and not wm[:, :off].any() and not wt.any()
        assert not dm[:, off + h * w:].any() and not dm[:, :off].any() and not dt.any(), (what, k)
        assert rel_linf(dm, wm) <= GRAD_TOL and rel_linf(du, wu) <= GRAD_TOL, (what, k)


@pytest.mark.parametrize("boundary_mode", mref.BOUNDARIES)
@pytest.mark.parametrize("scale", mref.LATTICE_SCALES)
def test_addressing_edges_at_every_level(scale, boundary_mode):
    """uv on the lattice of 32nds from -40/32 to 72/32: texel centres and borders of every level of (16, 8), exactly 0 and 1,
    negative remainders at the levels one texel wide; one footprint per case, so that every level and every pair is the one
    sampled in turn.  Ten slots sit on the range rule: x = 2^24 - 2 (the largest a slot can have) and -(2^24 - 2) are live,
    |x| = 2^24 is empty."""
    size, C = mref.LATTICE_SIZE, 5
    uv, da = mref.lattice_case(scale)
    uv, live = mref.range_case(uv)
    rng = np.random.default_rng(48)
    tex = rng.standard_normal(size + (C,), dtype=np.float32)
    tex[3, 2, :] = -0.0
    g = rng.standard_normal(mref.LATTICE_SHAPE + (C,), dtype=np.float32)
    out, (dt, dm, du), _ = _check(uv, da, tex, mref.mipmaps(tex), None, boundary_mode, None, g, ("lattice", scale, boundary_mode),
                                  zero="m" if scale == mref.LATTICE_SCALES[0] else "t" if scale >= 2 else "")
    for row in (0, 1):
        o, d = out[0, row, :5].reshape(10, C), du[0, row, :5].reshape(10, 2)
        assert not o[~live].any() and not d[~live].any() and np.abs(o[live]).max(-1).all()


@pytest.mark.parametrize("scale", mref.LATTICE_SCALES)
def test_every_sample_beyond_the_border_under_clamp(scale):
    """The lattice outside (0, 1) on both axes under clamp: the four taps of every level are one corner texel, dL/duv is exactly
    zero, and only the corners of the sampled levels receive a gradient."""
    size, C = mref.LATTICE_SIZE, 5
    uv, da = mref.lattice_case(scale, outside=True)
    rng = np.random.default_rng(49)
    tex = rng.standard_normal(size + (C,), dtype=np.float32)
    g = rng.standard_normal(mref.LATTICE_SHAPE + (C,), dtype=np.float32)
    st = mref.stage(uv, da, *size)
    _, (dt, dm, du), _ = _check(uv, da, tex, mref.mipmaps(tex), None, "clamp", None, g, ("outside", scale),
                                zero="mu" if scale == mref.LATTICE_SCALES[0] else "tu" if scale >= 2 else "u")
    rows = np.concatenate([dt.reshape(-1, C), dm])
    corners = np.zeros(len(rows), bool)
    for k, (h, w, off) in enumerate(mref.layout(*size)[1]):
        if ((st["j"] == k) | (st["two"] & (st["j"] + 1 == k))).any():
            corners[(0 if k == 0 else size[0] * size[1] + off) + np.array([0, w - 1, (h - 1) * w, h * w - 1])] = True
    assert corners.sum() in (2, 4, 6, 8) and not rows[~corners].any() and rows[corners].all()


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 5, 3, 8)])
def test_images_smaller_than_a_tile(shape):
    size, C = (16, 8), 3
    uv, da, rl = mref.case(shape, *size, seed=17)
    rng = np.random.default_rng(50)
    tex = rng.standard_normal((shape[0],) + size + (C,), dtype=np.float32)
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    single = int(np.prod(shape)) == 1                                        # one slot, magnified or not: one of the two tensors
    st = mref.stage(uv, da, *size, rl)
    assert not st["empty"].all()
    zero = "" if not single else "t" if st["j"].max() > 0 else "m" if not st["two"].any() else ""
    for boundary_mode in mref.BOUNDARIES:
        _check(uv, da, tex, mref.mipmaps(tex), rl, boundary_mode, None, g, ("small", shape, boundary_mode), zero=zero)


@pytest.mark.parametrize("mx", [0, 1, 2])
def test_max_mip_level_reaches_the_backward(mx):
    size, C = (16, 8), 5
    uv, da, rl = inputs(size)
    rng = np.random.default_rng(51 + mx)
    for per_view, boundary_mode in ((False, "wrap"), (True, "clamp")):
        tex = rng.standard_normal(((2,) if per_view else ()) + size + (C,), dtype=np.float32)
        mip = mref.mipmaps(tex, mx)
        assert mip.shape[-2] == (0, 32, 40)[mx]
        g = rng.standard_normal(SHAPE + (C,), dtype=np.float32)
        _check(uv, da, tex, mip, rl, boundary_mode, mx, g, ("max_mip_level", mx, per_view, boundary_mode))
