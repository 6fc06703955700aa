"""Renderer.texture / dm2_texture on the GPU against the contract's restatement (tests/texture_ref.py): the forward bit-equal
to forward32, both gradients within GRAD_TOL of grads64; the table-overflow route of the texel scatter and its opposite
(every lane on a few texels); borders; needs_input_grad; argument checks; the module path from rasterize to verts.grad; one
full-size case."""
import itertools

import numpy as np
import pytest
import torch

import interpolate_ref as iref
import rasterize_ref as rref
import texture_ref as ref
from util import GRAD_TOL, rel_linf, scenes, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

CS = (1, 2, 3, 4, 7, 16, 33)
LS = (1, 4, 8)
SIZES = ((1, 1), (5, 3), (64, 64), (300, 512), (2048, 2048))          # (Ht, Wt)
MODES = tuple(itertools.product(ref.FILTERS, ref.BOUNDARIES))
SOURCES = rref.SCENES + ("random",)
BMAX = 3


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


_UV = {}


def _uvs(source, L):
    """(render_layers or None, uv) as numpy: what rasterize + interpolate produce on rasterize_ref.scene(source) from a random
    per-vertex UV table in [-0.5, 1.5]^2 (-1 ids and zero UVs included), or random uv in [-2, 3]^2 without ids."""
    if (source, L) not in _UV:
        if source == "random":
            uv = np.random.RandomState(40 + L).uniform(-2, 3, (2, 40, 50, L, 2)).astype(np.float32)
            _UV[(source, L)] = (None, uv)
        else:
            s = rref.scene(source)
            layers, cnt, bary, t = _C.rasterize_layers_cuda(s["W"], s["H"], _cu(s["verts"]), _cu(s["faces"]), None, _cu(s["verts_ndc"]),
                                                            _cu(s["verts_image"]), _cu(s["ray_o"]), _cu(s["ray_d"]), L)
            table = np.random.RandomState(50 + L).uniform(-0.5, 1.5, (s["verts"].shape[0], 2)).astype(np.float32)
            uv = _C.interpolate_cuda(layers, bary, _cu(table), _cu(s["faces"]))
            _UV[(source, L)] = (layers.cpu().numpy(), uv.cpu().numpy())
    return _UV[(source, L)]


def _tex(rng, B, size, C, per_view):
    return rng.standard_normal(((B,) if per_view else ()) + tuple(size) + (C,), dtype=np.float32)


def _fwd(uv, tex, rl, filter_mode, boundary_mode):
    out = _C.texture_cuda(_cu(uv), _cu(tex), _cu(rl), filter_mode, boundary_mode)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bwd(uv, tex, rl, filter_mode, boundary_mode, g, need_tex=True, need_uv=True):
    dt, du = _C.texture_backward_cuda(_cu(uv), _cu(tex), _cu(rl), filter_mode, boundary_mode, _cu(g), need_tex, need_uv)
    torch.cuda.synchronize()
    return (None if dt is None else dt.cpu().numpy()), (None if du is None else du.cpu().numpy())


def _check_forward(uv, tex, rl, filter_mode, boundary_mode, what):
    got = _fwd(uv, tex, rl, filter_mode, boundary_mode)
    want = ref.forward32(uv, tex, rl, filter_mode, boundary_mode)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
    return got


def _check_grads(uv, tex, rl, filter_mode, boundary_mode, g, what, flat=False):
    """``flat``: the texture's neighbouring texels are equal by construction (one texel wide and high, or every sample beyond
    the border under clamp), so dL/duv is zero in the reference and must be exactly zero."""
    dt, du = _bwd(uv, tex, rl, filter_mode, boundary_mode, g)
    wt, wu = ref.grads64(uv, tex, rl, filter_mode, boundary_mode, g)
    assert dt.shape == tex.shape and du.shape == uv.shape, what
    et, eu = rel_linf(dt, wt), rel_linf(du, wu)
    print(what, "dtex", et, "duv", eu)
    assert np.abs(wt).max() > 0, what
    assert np.isfinite(dt).all() and et <= GRAD_TOL, (what, "dtex", et)
    if filter_mode == "nearest" or flat:
        assert not wu.any() and not du.any(), what
    else:
        assert np.abs(wu).max() > 0, what
        assert np.isfinite(du).all() and eu <= GRAD_TOL, (what, "duv", eu)
    assert (du[ref.empty(uv, tex.shape[-3], tex.shape[-2], rl)] == 0).all(), what
    return dt, du


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_forward_bit_equal_to_restatement(size, per_view):
    """Both filters x both boundary modes x CS x LS x SOURCES at this texture size and sharing."""
    rng = np.random.default_rng(100 + size[0])
    big = _tex(rng, BMAX, size, max(CS), per_view)
    big_gpu = _cu(big)
    stages = {}
    for C in CS:
        tex_c, tex_c_gpu = np.ascontiguousarray(big[..., :C]), big_gpu[..., :C].contiguous()
        for L, source in itertools.product(LS, SOURCES):
            rl, uv = _uvs(source, L)
            B = uv.shape[0]
            filled = int(uv[..., 0].size if rl is None else (rl >= 0).sum())
            if L == 4 and rl is not None:
                floor = {"soup": 50_000, "lattice": 15_000, "degenerate": 4_000, "no_faces": None}[source]
                assert filled == 0 if floor is None else filled > floor, (source, filled)
            tex, tex_gpu = (tex_c[:B], tex_c_gpu[:B]) if per_view else (tex_c, tex_c_gpu)
            uv_gpu, rl_gpu = _cu(uv), _cu(rl)
            for m in MODES:
                if (L, source, m) not in stages:
                    stages[(L, source, m)] = ref.stage(uv, size[0], size[1], rl, *m)
                got = _C.texture_cuda(uv_gpu, tex_gpu, rl_gpu, *m).cpu().numpy()
                want = ref.blend(stages[(L, source, m)], tex, m[0])
                what = (size, per_view, L, source, C, m)
                assert got.shape == uv.shape[:4] + (C,) and got.dtype == np.float32, what
                assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
                if source == "no_faces":
                    assert (got == 0).all()
                else:
                    assert 0.99 * filled <= (np.abs(got).max(-1) > 0).sum() <= filled, what
    del big, big_gpu


@pytest.mark.parametrize("k", range(2 * len(CS)))
def test_gradients_against_float64(k):
    """A thinned grid: every value of C, L, texture size, sharing, boundary mode and source appears with both filters."""
    C, per_view = CS[k // 2], bool(k % 2)
    boundary_mode, L, size, source = ref.BOUNDARIES[(k // 2) % 2], LS[k % 3], SIZES[k % 5], ("soup", "lattice", "random")[(k // 3) % 3]
    rl, uv = _uvs(source, L)
    rng = np.random.default_rng(200 + k)
    tex = _tex(rng, uv.shape[0], size, C, per_view)
    g = rng.standard_normal(uv.shape[:4] + (C,), dtype=np.float32)
    for filter_mode in ref.FILTERS:
        _check_forward(uv, tex, rl, filter_mode, boundary_mode, (k, filter_mode))
        _check_grads(uv, tex, rl, filter_mode, boundary_mode, g, (k, C, per_view, boundary_mode, L, size, source, filter_mode),
                     flat=size == (1, 1))


def test_gradient_grid_covers_every_axis():
    seen = [set() for _ in range(6)]
    for k in range(2 * len(CS)):
        for s, v in zip(seen, (CS[k // 2], bool(k % 2), ref.BOUNDARIES[(k // 2) % 2], LS[k % 3], SIZES[k % 5],
                               ("soup", "lattice", "random")[(k // 3) % 3])):
            s.add(v)
    assert [len(s) for s in seen] == [len(CS), 2, 2, len(LS), len(SIZES), 3]


@pytest.mark.parametrize("C", ref.INST_CS)
def test_every_instantiation_once(C):
    """Both filters x both boundary modes x shared and per-view textures at this C on texture_ref.instantiation_case() (the
    gradient grid above is thinned: C and the boundary mode move together there): every instantiation of the three kernels that
    C selects, at the smallest shape with two views, partial tiles, two layers and empty slots in every tile."""
    uv, rl = ref.instantiation_case()
    bad = ref.empty(uv, 5, 3, rl)
    rng = np.random.default_rng(700 + C)
    g = rng.standard_normal(uv.shape[:4] + (C,), dtype=np.float32)
    for per_view in (False, True):
        tex = _tex(rng, uv.shape[0], (5, 3), C, per_view)
        for filter_mode, boundary_mode in MODES:
            what = ("instantiation", C, per_view, filter_mode, boundary_mode)
            out = _check_forward(uv, tex, rl, filter_mode, boundary_mode, what)
            assert (out[bad] == 0).all(), what
            _check_grads(uv, tex, rl, filter_mode, boundary_mode, g, what)


@pytest.mark.parametrize("C", [3, 16])
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
def test_table_overflow_route(C, boundary_mode):
    """Random uv on a 2048^2 texture: every 16 x 16 tile addresses about 1024 distinct texels per layer, twice what the
    scatter's LDS table holds; the texels that find no slot add straight to global memory."""
    shape, size = (2, 48, 64, 4), (2048, 2048)
    rng = np.random.default_rng(5)
    uv = rng.uniform(0.0, 1.0, shape + (2,)).astype(np.float32)          # (beyond the border clamp would fold the samples)
    least = ref.distinct_texels_per_tile(uv, *size, None, "linear", boundary_mode)
    print("distinct texels per tile and layer, at least", least)
    assert least > table_capacity()
    rl = rng.integers(-1, 6, shape).astype(np.int32)
    for per_view in (False, True):
        tex = _tex(rng, shape[0], size, C, per_view)
        g = rng.standard_normal(shape + (C,), dtype=np.float32)
        for layers in (None, rl):
            _check_forward(uv, tex, layers, "linear", boundary_mode, ("overflow", C, per_view))
            _check_grads(uv, tex, layers, "linear", boundary_mode, g, ("overflow", C, per_view, layers is not None))
        _check_grads(uv, tex, None, "nearest", boundary_mode, g, ("overflow nearest", C, per_view))


@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_magnification_every_lane_on_a_few_texels(C, filter_mode):
    shape, size = (2, 50, 70, 4), (8, 8)
    rng = np.random.default_rng(6)
    uv = rng.uniform(0.32, 0.48, shape + (2,)).astype(np.float32)
    most = ref.distinct_texels_per_tile(uv, *size, None, filter_mode, "wrap", worst=max)
    print("distinct texels per tile and layer, at most", most)
    assert 0 < most < 16
    for per_view in (False, True):
        tex = _tex(rng, shape[0], size, C, per_view)
        g = rng.standard_normal(shape + (C,), dtype=np.float32)
        _check_forward(uv, tex, None, filter_mode, "wrap", ("magnified", C, per_view))
        _check_grads(uv, tex, None, filter_mode, "wrap", g, ("magnified", C, per_view))


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_borders(filter_mode):
    shape, C = (1, 33, 47, 2), 5
    rng = np.random.default_rng(7)
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    # clamp, every sample beyond the border: both corners of an axis on one texel
    side = rng.integers(0, 2, shape + (2,))
    uv = np.where(side == 1, rng.uniform(1.1, 2.0, shape + (2,)), rng.uniform(-1.0, -0.1, shape + (2,))).astype(np.float32)
    tex = _tex(rng, 1, (6, 9), C, False)
    _check_forward(uv, tex, None, filter_mode, "clamp", "outside")
    dt, _ = _check_grads(uv, tex, None, filter_mode, "clamp", g, "outside", flat=True)
    corners = np.zeros((6, 9), bool)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    assert (dt[~corners] == 0).all() and (dt[corners] != 0).all()
    # one texel wide / high, both modes: the two columns (rows) are the same texel and both add
    uv = rng.uniform(-2, 3, shape + (2,)).astype(np.float32)
    for size in ((1, 7), (7, 1), (1, 1)):
        tex = _tex(rng, 1, size, C, False)
        for boundary_mode in ref.BOUNDARIES:
            _check_forward(uv, tex, None, filter_mode, boundary_mode, (size, boundary_mode))
            dt, du = _check_grads(uv, tex, None, filter_mode, boundary_mode, g, (size, boundary_mode), flat=size == (1, 1))
            assert not du[..., 0 if size[1] == 1 else 1].any()


def test_empty_slots():
    """Negative ids, NaN / inf / 1e30 uv: zeros out, zero gradient, and texel (0, 0) -- where the zero uv of an empty slot
    points -- receives nothing from them."""
    shape, size, C = (2, 20, 30, 3), (4, 4), 3
    rng = np.random.default_rng(8)
    uv = rng.uniform(0.4, 0.8, shape + (2,)).astype(np.float32)          # x, y in [1.1, 2.7]: no good slot touches texel (0, 0)
    rl = rng.integers(0, 9, shape).astype(np.int32)
    bad = rng.uniform(size=shape) < 0.3
    kind = rng.integers(0, 6, shape)
    rl[bad & (kind == 0)] = -1
    uv[bad & (kind == 0)] = 0.0
    for k, val in ((1, np.nan), (2, np.inf), (3, -np.inf), (4, 1e30), (5, -1e30)):
        uv[bad & (kind == k), k % 2] = val
    assert np.array_equal(ref.empty(uv, *size, rl), bad) and bad.sum() > 300
    tex = _tex(rng, shape[0], size, C, False) + 10
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    for filter_mode, boundary_mode in MODES:
        out = _check_forward(uv, tex, rl, filter_mode, boundary_mode, "empty")
        assert (out[bad] == 0).all() and (out[~bad] != 0).all()
        dt, du = _check_grads(uv, tex, rl, filter_mode, boundary_mode, g, "empty")
        assert (du[bad] == 0).all() and (dt[0, 0] == 0).all()


def test_needs_input_grad():
    rl, uv = _uvs("lattice", 4)
    C, size = 6, (64, 64)
    rng = np.random.default_rng(9)
    tex = _tex(rng, 1, size, C, False)
    g = _cu(rng.standard_normal(uv.shape[:4] + (C,), dtype=np.float32))
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    calls = []
    real = _C.texture_backward_cuda

    def spy(*a):
        calls.append(tuple(a[-2:]))
        return real(*a)
    _C.texture_backward_cuda = spy
    try:
        res = {}
        for need_t, need_u in ((True, True), (True, False), (False, True)):
            t, u = _cu(tex).requires_grad_(need_t), _cu(uv).requires_grad_(need_u)
            out = r.texture(u, t, _cu(rl), boundary_mode="clamp")
            out.backward(g)
            res[(need_t, need_u)] = (None if t.grad is None else t.grad.clone(), None if u.grad is None else u.grad.clone())
        assert calls == [(True, True), (True, False), (False, True)]
        assert res[(True, False)][1] is None and res[(False, True)][0] is None
        # dL/duv is a pure function of the inputs: the same bits with and without the texture's gradient
        assert torch.equal(res[(True, True)][1], res[(False, True)][1])
        assert rel_linf(res[(True, False)][0].cpu().numpy(), res[(True, True)][0].cpu().numpy()) <= GRAD_TOL
        wt, wu = ref.grads64(uv, tex, rl, "linear", "clamp", g.cpu().numpy())
        assert np.abs(wt).max() > 0 and np.abs(wu).max() > 0
        assert rel_linf(res[(True, False)][0].cpu().numpy(), wt) <= GRAD_TOL
        assert rel_linf(res[(False, True)][1].cpu().numpy(), wu) <= GRAD_TOL
        del calls[:]
        launches = []
        lib = _C.load_library()
        real_b = lib.dm2_texture_backward
        lib.dm2_texture_backward = lambda *a: launches.append("b") or real_b(*a)
        try:
            out = r.texture(_cu(uv), _cu(tex), _cu(rl))
            assert out.grad_fn is None
            w = torch.ones(1, device="cuda", requires_grad=True)
            (out.sum() * w).backward()
            assert real(_cu(uv), _cu(tex), _cu(rl), "linear", "wrap", g, False, False) == (None, None)
        finally:
            lib.dm2_texture_backward = real_b
        assert not calls and not launches
    finally:
        _C.texture_backward_cuda = real


@pytest.mark.parametrize("C", [4, 16])
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_unaligned_tables_give_the_same_bits(C, filter_mode):
    """tex and the upstream gradient as views that start 4 bytes into their storage (no 16-byte alignment): the four-channel
    reads do not apply; the results are the same bits as with aligned tensors."""
    rl, uv = _uvs("soup", 4)
    rng = np.random.default_rng(13)
    tex = _tex(rng, 1, (64, 64), C, False)
    g = rng.standard_normal(uv.shape[:4] + (C,), dtype=np.float32)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = _cu(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    args, modes = (_cu(uv),), (_cu(rl), filter_mode, "wrap")
    out_a = _C.texture_cuda(*args, _cu(tex), *modes)
    out_u = _C.texture_cuda(*args, shifted(tex), *modes)
    dt_a, du_a = _C.texture_backward_cuda(*args, _cu(tex), *modes, _cu(g), True, True)
    dt_u, du_u = _C.texture_backward_cuda(*args, shifted(tex), *modes, shifted(g), True, True)
    assert torch.equal(out_a, out_u) and torch.equal(du_a, du_u)
    assert np.array_equal(_bits(out_u.cpu().numpy()), _bits(ref.forward32(uv, tex, rl, filter_mode, "wrap")))
    assert rel_linf(dt_u.cpu().numpy(), dt_a.cpu().numpy()) <= GRAD_TOL
    wt, wu = ref.grads64(uv, tex, rl, filter_mode, "wrap", g)
    assert rel_linf(dt_u.cpu().numpy(), wt) <= GRAD_TOL and rel_linf(du_u.cpu().numpy(), wu) <= GRAD_TOL


def test_argument_checks():
    uv = torch.zeros((2, 4, 5, 3, 2), device="cuda")
    tex = torch.zeros((8, 8, 3), device="cuda")
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32, device="cuda")
    ok = _C.texture_cuda(uv, tex, rl)
    assert tuple(ok.shape) == (2, 4, 5, 3, 3)
    for args, name in (((uv[..., :1], tex, rl), "uv"), ((uv[0], tex, rl[0]), "uv"), ((uv.double(), tex, rl), "uv"),
                       ((uv, tex[0], rl), "tex"), ((uv, tex[None].expand(3, 8, 8, 3), rl), "tex"), ((uv, tex[:0], rl), "tex"),
                       ((uv, tex[..., :0], rl), "tex"), ((uv, tex.half(), rl), "tex"),
                       ((uv, tex, rl[:1]), "render_layers"), ((uv, tex, rl.long()), "render_layers")):
        with pytest.raises(RuntimeError, match=name):
            _C.texture_cuda(*args)
    with pytest.raises(RuntimeError, match="filter_mode"):
        _C.texture_cuda(uv, tex, rl, "cubic", "wrap")
    with pytest.raises(RuntimeError, match="boundary_mode"):
        _C.texture_cuda(uv, tex, rl, "linear", "mirror")
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.texture_backward_cuda(uv, tex, rl, "linear", "wrap", ok[..., :2], True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_cuda(uv.cpu(), tex.cpu(), rl.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_cuda(uv, tex.cpu(), rl)
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    with pytest.raises(RuntimeError, match="filter_mode"):
        r.texture(uv, tex, rl, filter_mode="trilinear")
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    p = lambda t: _C._ptr(t)
    assert lib.dm2_texture(2, 4, 5, 3, 8, 8, 3, 0, 2, 0, p(rl), p(uv), p(tex), p(ok), None) == 1
    assert lib.dm2_texture(2, 4, 5, 3, 8, 8, 3, 0, 1, 7, p(rl), p(uv), p(tex), p(ok), None) == 1
    assert lib.dm2_texture(2, 4, 5, 3, 0, 8, 3, 0, 1, 0, p(rl), p(uv), p(tex), p(ok), None) == 1
    assert lib.dm2_texture(2, 4, 5, 3, 65536, 65536, 3, 0, 1, 0, p(rl), p(uv), p(tex), p(ok), None) == 1
    assert lib.dm2_texture(2, 4, 5, 3, 8, 8, 3, 0, 1, 0, p(rl), None, p(tex), p(ok), None) == 1


def test_degenerate_sizes():
    tex = _cu(_tex(np.random.default_rng(10), 1, (4, 4), 3, False))
    launches = []
    lib = _C.load_library()
    real_f, real_b = lib.dm2_texture, lib.dm2_texture_backward
    try:
        lib.dm2_texture = lambda *a: launches.append("f") or real_f(*a)
        lib.dm2_texture_backward = lambda *a: launches.append("b") or real_b(*a)
        for shape in ((0, 4, 5, 2), (2, 0, 5, 2), (2, 4, 0, 2), (2, 4, 5, 0)):
            uv = torch.zeros(shape + (2,), device="cuda")
            rl = torch.zeros(shape, dtype=torch.int32, device="cuda")
            for layers in (None, rl):
                out = _C.texture_cuda(uv, tex, layers)
                assert tuple(out.shape) == shape + (3,) and out.dtype == torch.float32
                dt, du = _C.texture_backward_cuda(uv, tex, layers, "linear", "wrap", torch.ones_like(out), True, True)
                assert tuple(dt.shape) == tuple(tex.shape) and tuple(du.shape) == shape + (2,) and (dt == 0).all()
        assert not launches
    finally:
        lib.dm2_texture, lib.dm2_texture_backward = real_f, real_b


def _module_scene(name, W, H):
    if name == "lattice":
        ts = scenes.tet_lattice(W, H, 4, seed=scenes.SEED_BASE + 84, num_cams=2).to("cuda")
        return ts.mv, ts.proj, ts.verts, ts.faces
    sc = scenes.triangle_soup(W, H, 600, scenes.SEED_BASE + 85, num_cams=2, depth_complexity=12.0, shared_verts=True).to("cuda")
    return sc.mv, sc.proj, sc.verts, sc.faces


@pytest.mark.parametrize("name", ["lattice", "soup"])
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
def test_module_path_end_to_end(name, boundary_mode):
    """rasterize -> interpolate (a UV table with an attr_faces of its own: three rows per face) -> texture -> a random-weighted
    sum: tex.grad against texture_ref.grads64, verts.grad and the UV table's gradient against interpolate_ref.grads64 +
    rasterize_ref.grads64 fed the float64 dL/duv."""
    W, H, bidx, L, C, size = 80, 64, [1, 0], 4, 3, (64, 64)
    mv, proj, verts0, faces = _module_scene(name, W, H)
    r = dm2.LayeredRenderer(mv, proj, W, H, "cuda")
    assert type(r).texture is dm2.Renderer.texture                       # inherited
    ro, rd = r._camera_rows(r.ray_o, bidx).cpu().numpy(), r._camera_rows(r.ray_d, bidx).cpu().numpy()
    gen = torch.Generator().manual_seed(11)
    F = faces.shape[0]
    uv_faces = torch.arange(3 * F, dtype=torch.int32).reshape(F, 3).cuda()
    table0 = (torch.rand((3 * F, 2), generator=gen) * 2 - 0.5).cuda()
    tex0 = torch.randn(size + (C,), generator=gen).cuda()
    verts, table, tex = (x.clone().requires_grad_(True) for x in (verts0, table0, tex0))
    layers, cnt, bary, t = r.rasterize(bidx, verts, faces, L)
    uv = r.interpolate(layers, bary, table, uv_faces)
    out = r.texture(uv, tex, layers, boundary_mode=boundary_mode)
    wgt = torch.randn(out.shape, generator=gen).cuda()
    (out * wgt).sum().backward()
    assert int(cnt.sum()) > 3000
    rl, bn, un, tn, gn = (x.detach().cpu().numpy() for x in (layers, bary, uv, tex0, wgt))
    assert np.array_equal(_bits(un), _bits(iref.forward32(rl, bn, table0.cpu().numpy(), uv_faces.cpu().numpy())))
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(ref.forward32(un, tn, rl, "linear", boundary_mode)))
    wt, wu = ref.grads64(un, tn, rl, "linear", boundary_mode, gn)
    wtab, wb = iref.grads64(rl, bn, table0.cpu().numpy(), uv_faces.cpu().numpy(), wu)
    wv = rref.grads64(verts0.cpu().numpy(), faces.cpu().numpy(), rl, ro, rd, wb, None)
    et, ea, ev = rel_linf(tex.grad.cpu().numpy(), wt), rel_linf(table.grad.cpu().numpy(), wtab), rel_linf(verts.grad.cpu().numpy(), wv)
    print(name, boundary_mode, "tex.grad", et, "uv table grad", ea, "verts.grad", ev)
    assert np.abs(wt).max() > 0 and np.abs(wtab).max() > 0 and np.abs(wv).max() > 0
    assert et <= GRAD_TOL and ea <= GRAD_TOL and ev <= GRAD_TOL


def test_cfg3_full_size():
    """SURVEY.md 8(d) cfg 3: tet_lattice(n=25) at 1024^2, L = 4; C = 3, a 2048^2 texture."""
    ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to("cuda")
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, "cuda")
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        layers, cnt, bary, t = lr.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
        table = torch.rand((ts.verts.shape[0], 2), generator=gen).cuda()
        uv0 = lr.interpolate(layers, bary, table, ts.faces)
    tex = torch.randn((2048, 2048, 3), generator=gen).cuda().requires_grad_(True)
    uv = uv0.clone().requires_grad_(True)
    out = lr.texture(uv, tex, layers)
    g = torch.randn(out.shape, generator=gen).cuda()
    out.backward(g)
    rl, un, tn = (x.detach().cpu().numpy() for x in (layers, uv0, tex))
    assert int((rl >= 0).sum()) > 500_000
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(ref.forward32(un, tn, rl, "linear", "wrap")))
    wt, wu = ref.grads64(un, tn, rl, "linear", "wrap", g.cpu().numpy())
    et, eu = rel_linf(tex.grad.cpu().numpy(), wt), rel_linf(uv.grad.cpu().numpy(), wu)
    print("cfg3 dtex", et, "duv", eu)
    assert np.abs(wt).max() > 0 and np.abs(wu).max() > 0
    assert et <= GRAD_TOL and eu <= GRAD_TOL
    assert (uv.grad[layers < 0] == 0).all()
