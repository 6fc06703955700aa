"""Renderer.texture3d / dm2_texture_volume on the GPU against the contract's restatement
(tests/texture_volume_ref.py): the forward bit-equal to forward32, both gradients per element within
|g - g64| <= 1e-5 max|g64| + 8 eps32 sum|terms| (util.summation_bound) with exact zeros where no term arrives; the two routes of
the voxel scatter; empty slots next to a NaN-poisoned grid; alignment and strides; needs_input_grad; repeats; the argument checks
down to the C ABI; the module path from rasterize to verts.grad, and torch's grid_sample in texture3d's place."""
import functools

import numpy as np
import pytest
import torch

import texture_volume_ref as ref
from util import scenes, summation_bound, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, BIDX = 40, 24, [1, 0]            # no multiple of the 16 x 16 tile either way: partial tiles on both axes
NS = (1, 2, 5, 16)
CS = (1, 2, 3, 4, 5, 8, 16)           # every chunk length of the scatter (1, 2, 3, 4, 4 + 1), the four-channel reads at 4, 8 and 16
LS = (1, 3)
CLAMP, WRAP = _C.TEX_BOUNDARIES["clamp"], _C.TEX_BOUNDARIES["wrap"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene():
    return scenes.tet_lattice(W, H, 3, seed=scenes.SEED_BASE + 91, num_cams=2)


@functools.lru_cache(maxsize=None)
def _coords(source, L):
    """(render_layers or None, xyz) as numpy, computed once.  "lattice": rasterize + shading_vectors on a small tet lattice,
    the positions mapped by (position - lo) / (hi - lo) with a box shifted against the mesh's bounds, so that some hits lie outside
    the unit cube; empty slots (-1 ids) hold what the map makes of the zeros shading_vectors writes.  "random": uniform in [-0.4, 1.4]^3, no ids."""
    if source == "random":
        return None, np.random.default_rng(40 + L).uniform(-0.4, 1.4, (2, H, W, L, 3)).astype(f32)
    ts = _scene().to("cuda")
    r = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda")
    layers, cnt, bary, t = r.rasterize(BIDX, ts.verts, ts.faces, L)
    pos = r.shading_vectors(BIDX, layers, t)[0]
    lo, hi = ts.verts.min(0).values, ts.verts.max(0).values
    mid = pos[layers >= 0].median(0).values                              # (a box 0.8 of the mesh's extent round the hits' median,
    lo, hi = mid - 0.35 * (hi - lo), mid + 0.45 * (hi - lo)              # off centre: some hits inside it, some beyond either side)
    xyz = (pos - lo) / (hi - lo)
    rl, p = _np(layers), _np(xyz)
    live = rl >= 0
    assert live.sum() > 200 and (~live).any() and not _np(pos)[~live].any()
    outside = ((p < 0) | (p > 1)).any(-1) & live
    print(source, L, "live", int(live.sum()), "outside the unit cube", int(outside.sum()))
    assert outside.sum() > 20 and (live & ~outside).sum() > 20
    return rl, p


def _grid(rng, B, N, C, per_view):
    return rng.standard_normal(((B,) if per_view else ()) + (N, N, N, C), dtype=f32)


def _fwd(p, grid, rl, filter_mode, boundary_mode):
    out = _C.texture_volume_cuda(_cu(p), _cu(grid), _cu(rl), filter_mode, boundary_mode)
    torch.cuda.synchronize()
    return _np(out)


def _bwd(p, grid, rl, filter_mode, boundary_mode, g, need_grid=True, need_xyz=True):
    dg, dp = _C.texture_volume_backward_cuda(_cu(p), _cu(grid), _cu(rl), filter_mode, boundary_mode, _cu(g), need_grid, need_xyz)
    torch.cuda.synchronize()
    return _np(dg), _np(dp)


def _check_forward(p, grid, rl, filter_mode, boundary_mode, what):
    got = _fwd(p, grid, rl, filter_mode, boundary_mode)
    want = ref.forward32(p, grid, rl, filter_mode, boundary_mode)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
    return got


WORST = {}


def _check_grads(p, grid, rl, filter_mode, boundary_mode, g, what):
    """Per element within util.summation_bound of grads64; exact zeros where no term arrives -> (dL/dgrid, dL/dxyz)."""
    dg, dp = _bwd(p, grid, rl, filter_mode, boundary_mode, g)
    wg, wp = ref.grads64(p, grid, rl, filter_mode, boundary_mode, g)
    sg, sp = ref.terms_abs(p, grid, rl, filter_mode, boundary_mode, g)
    assert dg.shape == np.shape(grid) and dp.shape == np.shape(p), what
    assert np.isfinite(dg).all() and np.isfinite(dp).all(), what
    assert np.abs(wg).max() > 0, what
    for name, got, want, sabs in (("grid", dg, wg, sg), ("xyz", dp, wp, sp)):
        err, bound = np.abs(got - want), summation_bound(float(np.abs(want).max()), sabs)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        WORST[name] = max(WORST.get(name, 0.0), ratio)
        print(what, name, "worst err / bound", ratio)
        assert (err <= bound).all(), (what, name, ratio)
        assert not got[sabs == 0].any(), (what, name)                     # no term: exactly zero
    if filter_mode == "nearest":
        assert not wp.any() and not dp.any(), what
    assert not dp[ref.empty(p, np.shape(grid)[-2], rl)].any(), what
    return dg, dp


@pytest.mark.parametrize("C", CS)
def test_forward_and_gradients(C):
    """N x filter x boundary at this C; shared or per-view grid, L and the source of the coordinates rotate through their eight
    combinations (twice per C), so every instantiation of the three kernels that C selects runs on both kinds of input."""
    rng = np.random.default_rng(100 + C)
    combos = [(pv, L, src) for pv in (False, True) for L in LS for src in ("lattice", "random")]
    seen, k = set(), C
    for N in NS:
        for filter_mode in ref.FILTERS:
            for boundary_mode in ref.BOUNDARIES:
                per_view, L, source = combos[k % 8]
                k += 3                                                    # (3 and 8 coprime: all eight combinations in any eight steps)
                seen.add((per_view, L, source))
                rl, p = _coords(source, L)
                grid = _grid(rng, p.shape[0], N, C, per_view)
                g = rng.standard_normal(p.shape[:4] + (C,), dtype=f32)
                what = (C, N, filter_mode, boundary_mode, per_view, L, source)
                out = _check_forward(p, grid, rl, filter_mode, boundary_mode, what)
                if rl is not None:
                    assert not out[rl < 0].any(), what
                _, dp = _check_grads(p, grid, rl, filter_mode, boundary_mode, g, what)
                if filter_mode == "linear" and N > 1:
                    assert np.abs(dp).max() > 0, what
    assert len(seen) == 8
    print("worst err / bound so far", WORST)


@pytest.mark.parametrize("C", [3, 16])
def test_table_overflow_route(C):
    """One 16 x 16 tile of unrelated positions in a 32^3 grid: about 2000 distinct voxels in the tile's layer, four times what
    the scatter's table holds, so most contributions go straight to global memory; next to it a coherent surface (a slightly
    tilted plane across a few voxels) whose voxels all find a slot."""
    N, shape = 32, (1, 16, 16, 1)
    rng = np.random.default_rng(5)
    scattered = rng.uniform(0, 1, shape + (3,)).astype(f32)
    yy, xx = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    plane = np.stack([0.3 + xx / 16 * 0.2, 0.4 + yy / 16 * 0.2, 0.5 + 0.01 * xx + 0.005 * yy], -1).reshape(shape + (3,)).astype(f32)
    n_scattered = ref.distinct_voxels_per_tile(scattered, N)
    n_plane = ref.distinct_voxels_per_tile(plane, N, worst=max)
    print("distinct voxels: scattered", n_scattered, "plane", n_plane, "table", table_capacity())
    assert n_scattered > 2 * table_capacity() and 8 < n_plane < table_capacity() // 2
    for p in (scattered, plane):
        for per_view in (False, True):
            grid = _grid(rng, 1, N, C, per_view)
            g = rng.standard_normal(shape + (C,), dtype=f32)
            for boundary_mode in ref.BOUNDARIES:
                _check_forward(p, grid, None, "linear", boundary_mode, ("overflow", C, per_view))
                _check_grads(p, grid, None, "linear", boundary_mode, g, ("overflow", C, per_view, boundary_mode))
            _check_grads(p, grid, None, "nearest", "clamp", g, ("overflow nearest", C, per_view))


@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_empty_slots_next_to_a_poisoned_grid(filter_mode, boundary_mode):
    """Negative ids over the zeros shading_vectors writes, NaN, infinities, coordinates beyond the 2^24 rule, on one axis at a
    time: zeros out, zero gradient, nothing added to the grid.  The live slots stay in [0.3, 0.9]^3 of an 8^3 grid, so nobody
    reads the voxels of index 0 on any axis, which hold NaN: an empty slot that sampled (0, 0, 0) would show."""
    shape, N, C = (2, 20, 30, 3), 8, 3
    rng = np.random.default_rng(8)
    p = rng.uniform(0.3, 0.9, shape + (3,)).astype(f32)
    rl = rng.integers(0, 9, shape).astype(np.int32)
    bad = rng.uniform(size=shape) < 0.3
    kind = rng.integers(0, 6, shape)
    rl[bad & (kind == 0)] = -1
    p[bad & (kind == 0)] = (0.0, -0.0, 0.0)
    for k, val in ((1, np.nan), (2, np.inf), (3, -np.inf), (4, 2.0 ** 24 / N + 1.0), (5, -(2.0 ** 24) / N)):
        p[bad & (kind == k), k % 3] = val
    assert np.array_equal(ref.empty(p, N, rl), bad) and bad.sum() > 300
    grid = _grid(rng, shape[0], N, C, False) + 10
    grid[0, :, :], grid[:, 0, :], grid[:, :, 0] = np.nan, np.nan, np.nan
    g = rng.standard_normal(shape + (C,), dtype=f32)
    out = _check_forward(p, grid, rl, filter_mode, boundary_mode, "empty")
    assert (out[bad] == 0).all() and (out[~bad] != 0).all() and np.isfinite(out).all()
    dg, dp = _check_grads(p, grid, rl, filter_mode, boundary_mode, g, "empty")
    assert (dp[bad] == 0).all()
    assert not dg[0, :, :].any() and not dg[:, 0, :].any() and not dg[:, :, 0].any()
    # all-ones upstream: the grid receives exactly one unit of weight per live slot and channel
    dg1, _ = _bwd(p, grid, rl, filter_mode, boundary_mode, np.ones_like(g))
    assert np.allclose(dg1.sum((0, 1, 2)), (~bad).sum(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("C", [4, 8])
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_unaligned_and_strided_inputs_give_the_same_bits(C, filter_mode):
    """The grid and the upstream gradient as views that start 4 bytes into their storage (no 16-byte alignment: the
    four-channel reads do not apply), and xyz / grid / grad_out as non-contiguous views: the same bits as the plain call."""
    N = 5
    rl, p = _coords("lattice", 3)
    rng = np.random.default_rng(13)
    grid = _grid(rng, 1, N, C, False)
    g = rng.standard_normal(p.shape[:4] + (C,), dtype=f32)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = _cu(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    def strided(a):
        wide = torch.zeros(a.shape[:-1] + (2 * a.shape[-1],), dtype=torch.float32, device="cuda")
        wide[..., ::2] = _cu(a)
        v = wide[..., ::2]
        assert not v.is_contiguous()
        return v
    for boundary_mode in ref.BOUNDARIES:
        modes = (_cu(rl), filter_mode, boundary_mode)
        out_a = _C.texture_volume_cuda(_cu(p), _cu(grid), *modes)
        dg_a, dp_a = _C.texture_volume_backward_cuda(_cu(p), _cu(grid), *modes, _cu(g), True, True)
        assert np.array_equal(_bits(_np(out_a)), _bits(ref.forward32(p, grid, rl, filter_mode, boundary_mode)))
        wg, wp = ref.grads64(p, grid, rl, filter_mode, boundary_mode, g)
        sg, _ = ref.terms_abs(p, grid, rl, filter_mode, boundary_mode, g)
        for how in (shifted, strided):
            out_u = _C.texture_volume_cuda(how(p) if how is strided else _cu(p), how(grid), *modes)
            dg_u, dp_u = _C.texture_volume_backward_cuda(how(p) if how is strided else _cu(p), how(grid), *modes, how(g), True, True)
            assert torch.equal(out_a, out_u) and torch.equal(dp_a, dp_u), how.__name__
            assert (np.abs(_np(dg_u) - wg) <= summation_bound(float(np.abs(wg).max()), sg)).all(), how.__name__


def test_needs_input_grad_and_repeats():
    """Only what requires grad is computed (one output pointer NULL in the C call), nothing launches when nothing is wanted,
    and dL/dxyz is the same bits on every call and with or without the grid's gradient beside it."""
    rl, p = _coords("lattice", 3)
    C, N = 6, 5
    rng = np.random.default_rng(9)
    grid = _grid(rng, 1, N, C, False)
    g = _cu(rng.standard_normal(p.shape[:4] + (C,), dtype=f32))
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    lib = _C.load_library()
    real_b = lib.dm2_texture_volume_backward
    calls = []

    def spy(*a):
        calls.append((a[7:9], a[-3].value is not None, a[-2].value is not None))     # ((filter, boundary), dL_dgrid, dL_dxyz not NULL)
        return real_b(*a)
    lib.dm2_texture_volume_backward = spy
    try:
        res = {}
        for need_g, need_p in ((True, True), (True, False), (False, True), (True, True)):
            t, u = _cu(grid).requires_grad_(need_g), _cu(p).requires_grad_(need_p)
            out = r.texture3d(u, t, _cu(rl), boundary_mode="wrap")
            out.backward(g)
            res.setdefault((need_g, need_p), []).append((t.grad, u.grad))
        code = (_C.TEX_FILTERS["linear"], WRAP)
        assert calls == [(code, True, True), (code, True, False), (code, False, True), (code, True, True)]
        assert res[(True, False)][0][1] is None and res[(False, True)][0][0] is None
        first, again = res[(True, True)]
        assert torch.equal(first[1], again[1]) and torch.equal(first[1], res[(False, True)][0][1])
        wg, wp = ref.grads64(p, grid, rl, "linear", "wrap", _np(g))
        sg, sp = ref.terms_abs(p, grid, rl, "linear", "wrap", _np(g))
        assert np.abs(wg).max() > 0 and np.abs(wp).max() > 0
        assert (np.abs(_np(res[(True, False)][0][0]) - wg) <= summation_bound(float(np.abs(wg).max()), sg)).all()
        assert (np.abs(_np(res[(False, True)][0][1]) - wp) <= summation_bound(float(np.abs(wp).max()), sp)).all()
        del calls[:]
        out = r.texture3d(_cu(p), _cu(grid), _cu(rl))
        assert out.grad_fn is None
        w = torch.ones(1, device="cuda", requires_grad=True)
        (out.sum() * w).backward()
        assert _C.texture_volume_backward_cuda(_cu(p), _cu(grid), _cu(rl), "linear", "clamp", g, False, False) == (None, None)
        assert not calls
    finally:
        lib.dm2_texture_volume_backward = real_b


def test_argument_checks():
    p = torch.full((2, 4, 5, 3, 3), 0.5, device="cuda")
    grid = torch.zeros((8, 8, 8, 3), device="cuda")
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32, device="cuda")
    ok = _C.texture_volume_cuda(p, grid, rl)
    assert tuple(ok.shape) == (2, 4, 5, 3, 3)
    for args, name in (((p[..., :2], grid, rl), "xyz"), ((p.double(), grid, rl), "xyz"), ((p, grid[:7], rl), "grid"),
                       ((p, grid.half(), rl), "grid"), ((p, grid, rl[:1]), "render_layers"), ((p, grid, rl.long()), "render_layers")):
        with pytest.raises(RuntimeError, match=name):
            _C.texture_volume_cuda(*args)
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.texture_volume_backward_cuda(p, grid, rl, "linear", "clamp", ok.double(), True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_volume_cuda(p, grid.cpu(), rl)
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    with pytest.raises(ValueError, match="filter_mode"):
        r.texture3d(p, grid, rl, filter_mode="cubic")
    with pytest.raises(ValueError, match="boundary_mode"):
        r.texture3d(p, grid, rl, boundary_mode="mirror")
    assert torch.equal(r.texture3d(p.double(), grid, rl.long()), ok)       # (the method converts dtypes, as texture does)
    # degenerate sizes: no launch
    for shape in ((0, 4, 5, 2), (2, 4, 5, 0)):
        e = torch.ones(shape + (3,), device="cuda")
        out = _C.texture_volume_cuda(e, grid)
        dg, dp = _C.texture_volume_backward_cuda(e, grid, None, "linear", "clamp", torch.ones_like(out), True, True)
        assert tuple(out.shape) == shape + (3,) and tuple(dg.shape) == tuple(grid.shape) and tuple(dp.shape) == shape + (3,) and not dg.any()
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    q = lambda t: _C._ptr(t)
    lin = _C.TEX_FILTERS["linear"]
    dp = torch.empty_like(p)
    nearest = _C.TEX_FILTERS["nearest"]
    fwd = lambda N, f, b, xyz=p: lib.dm2_texture_volume(2, 4, 5, 3, N, 3, 0, f, b, q(rl), q(xyz) if xyz is not None else None, q(grid),
                                                        q(ok), None)
    bwd = lambda N, f, b, xyz=p: lib.dm2_texture_volume_backward(2, 4, 5, 3, N, 3, 0, f, b, q(rl), q(xyz) if xyz is not None else None,
                                                                 q(grid), q(ok), q(grid), q(dp), None)
    cube = lambda f: lib.dm2_texture_cube(2, 4, 5, 3, 8, 3, 0, f, q(rl), q(p), q(grid), q(ok), None)
    cube_b = lambda f: lib.dm2_texture_cube_backward(2, 4, 5, 3, 8, 3, 0, f, q(rl), q(p), q(grid), q(ok), q(grid), q(dp), None)
    for call, old in ((fwd, cube), (bwd, cube_b)):
        for f, b in ((lin, CLAMP), (lin, WRAP), (nearest, CLAMP), (nearest, WRAP)):
            assert call(8, f, b) == 0, (f, b)
        assert call(0, lin, CLAMP) == 1
        assert call(1291, lin, CLAMP) == 1                                # 1291^3 >= 2^31 > 1290^3
        assert call(2 ** 31 - 1, lin, WRAP) == 1
        assert call(8, lin, 2) == 1 and call(8, lin, -1) == 1             # an unknown boundary
        for unknown in (2, 4, 0x80, 0x400, 0x40000000):
            assert call(8, lin | unknown, CLAMP) == 1, unknown            # an unknown filter
            assert old(lin | unknown) == 1, unknown                       # (and of the cube's own symbol, as before)
        assert old(0x101) == 1 and old(0x201) == 1                        # ABI 7's volume codes: unknown filters of the cube now
        assert call(8, lin, CLAMP, None) == 1                             # NULL xyz
    torch.cuda.synchronize()
    assert not _np(grid).any()                                            # (the accepted backward calls added g = ok = 0)


def test_module_path_end_to_end():
    """rasterize -> shading_vectors -> (position - lo) / (hi - lo) -> texture3d -> composite -> a random-weighted sum: finite,
    non-zero grid.grad and verts.grad; the forward bit-equal to forward32; the same forward with torch's grid_sample (clamp =
    padding_mode "border") in texture3d's place within 1e-5 of the maximum."""
    Wm, Hm, bidx, L, C, N = 80, 64, [1, 0], 4, 3, 16
    ts = scenes.tet_lattice(Wm, Hm, 4, seed=scenes.SEED_BASE + 84, num_cams=2).to("cuda")
    r = dm2.LayeredRenderer(ts.mv, ts.proj, Wm, Hm, "cuda")
    assert type(r).texture3d is dm2.Renderer.texture3d                   # inherited
    gen = torch.Generator().manual_seed(11)
    grid0 = torch.randn((N, N, N, C), generator=gen).cuda()
    alpha0 = torch.rand((ts.faces.shape[0],), generator=gen).cuda() * 0.8 + 0.1
    bg = torch.tensor([0.2, -0.1, 0.5]).cuda()
    verts, grid = ts.verts.clone().requires_grad_(True), grid0.clone().requires_grad_(True)
    layers, cnt, bary, t = r.rasterize(bidx, verts, ts.faces, L)
    pos = r.shading_vectors(bidx, layers, t)[0]
    lo, hi = ts.verts.min(0).values, ts.verts.max(0).values
    xyz = (pos - lo) / (hi - lo)
    shaded = r.texture3d(xyz, grid, layers)
    out, acc = r.composite(shaded, alpha0, layers, bg)
    wgt = torch.randn(out.shape, generator=gen).cuda()
    (out * wgt).sum().backward()
    assert int(cnt.sum()) > 3000
    for x in (grid.grad, verts.grad):
        assert x is not None and torch.isfinite(x).all() and x.abs().max() > 0
    rl, pn = _np(layers), _np(xyz)
    assert np.array_equal(_bits(_np(shaded)), _bits(ref.forward32(pn, _np(grid0), rl, "linear", "clamp")))
    # the lines texture3d replaces
    vol = grid0.permute(3, 0, 1, 2)[None].expand(len(bidx), -1, -1, -1, -1)
    gs = torch.nn.functional.grid_sample(vol, 2.0 * xyz.detach() - 1.0, mode="bilinear", padding_mode="border", align_corners=False)
    gs = gs.permute(0, 2, 3, 4, 1) * (layers >= 0)[..., None]
    out_gs, _ = r.composite(gs.contiguous(), alpha0, layers, bg)
    err = float((out_gs - out.detach()).abs().max() / out.detach().abs().max())
    print("composite over grid_sample against composite over texture3d", err)
    assert err <= 1e-5
