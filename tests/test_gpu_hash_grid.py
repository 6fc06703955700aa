"""Renderer.hash_grid / dm2_hash_grid on the GPU against the contract's restatement
(tests/hash_grid_ref.py): the forward bit-equal to forward32, both gradients per element within
|g - g64| <= 1e-5 max|g64| + 8 eps32 sum|terms| (util.summation_bound) with exact zeros where no term arrives; a single dense level
against texture3d's kernels; the two routes of the table scatter; empty slots next to a NaN-poisoned table; alignment and strides;
needs_input_grad; repeats; sparse upstream gradients; the argument checks down to the C ABI; the module path from rasterize to
verts.grad, and the plain-torch encoding in hash_grid's place."""
import functools

import numpy as np
import pytest
import torch

import hash_grid_ref as ref
import upstream as U
from util import scenes, summation_bound, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, BIDX = 40, 24, [1, 0]            # no multiple of the 16 x 16 tile either way: partial tiles on both axes
FS = (1, 2, 4, 8)
LS = (1, 3)
# (N, q, NL, T): levels 0-2 dense and 3-4 hashed and colliding (2, 3, 4, 6, 9 on 64 rows); R = 1 first (1, 2, 4, 8 on 16 rows:
# two dense, two hashed); equal resolutions with separate tables (5, 5, 5, dense); all hashed (16, 24, 36, 54 on 1024 rows)
CFGS = ((2, 24, 5, 64), (1, 32, 4, 16), (5, 17, 3, 256), (16, 24, 4, 1024))


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
    the unit cube; empty slots (-1 ids) hold what the map makes of the zeros shading_vectors writes.  "random": uniform in
    [-0.4, 1.4]^3, no ids."""
    if source == "random":
        return None, np.random.default_rng(40 + L).uniform(-0.4, 1.4, (2, H, W, L, 3)).astype(f32)
    ts = _scene().to("cuda")
    r = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda")
    layers, cnt, bary, t = r.rasterize(BIDX, ts.verts, ts.faces, L)
    pos = r.shading_vectors(BIDX, layers, t)[0]
    lo, hi = ts.verts.min(0).values, ts.verts.max(0).values
    mid = pos[layers >= 0].median(0).values
    lo, hi = mid - 0.35 * (hi - lo), mid + 0.45 * (hi - lo)
    xyz = (pos - lo) / (hi - lo)
    rl, p = _np(layers), _np(xyz)
    live = rl >= 0
    assert live.sum() > 200 and (~live).any() and not _np(pos)[~live].any()
    outside = ((p < 0) | (p > 1)).any(-1) & live
    assert outside.sum() > 20 and (live & ~outside).sum() > 20
    return rl, p


def _table(rng, NL, T, F):
    return rng.standard_normal((NL, T, F), dtype=f32)


def _fwd(p, table, rl, N, q, filter_mode, boundary_mode):
    out = _C.hash_grid_cuda(_cu(p), _cu(table), _cu(rl), N, q / 16, filter_mode, boundary_mode)
    torch.cuda.synchronize()
    return _np(out)


def _bwd(p, table, rl, N, q, filter_mode, boundary_mode, g, need_table=True, need_xyz=True):
    dt, dp = _C.hash_grid_backward_cuda(_cu(p), _cu(table), _cu(rl), N, q / 16, filter_mode, boundary_mode, _cu(g), need_table, need_xyz)
    torch.cuda.synchronize()
    return _np(dt), _np(dp)


def _check_forward(p, table, rl, N, q, filter_mode, boundary_mode, what):
    got = _fwd(p, table, rl, N, q, filter_mode, boundary_mode)
    want = ref.forward32(p, table, rl, N, q, filter_mode, boundary_mode)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
    return got


WORST = {}


def _check_against(what, dt, dp, p, table, rl, N, q, filter_mode, boundary_mode, g):
    wt, wp = ref.grads64(p, table, rl, N, q, filter_mode, boundary_mode, g)
    st, sp = ref.terms_abs(p, table, rl, N, q, filter_mode, boundary_mode, g)
    pairs = []
    if dt is not None:
        assert dt.shape == np.shape(table), what
        pairs.append(("table", dt, wt, st))
    if dp is not None:
        assert dp.shape == np.shape(p), what
        pairs.append(("xyz", dp, wp, sp))
    for name, got, want, sabs in pairs:
        assert np.isfinite(got).all(), (what, name)
        err, bound = np.abs(got - want), summation_bound(float(np.abs(want).max()), sabs)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        WORST[name] = max(WORST.get(name, 0.0), ratio)
        print(what, name, "worst err / bound", ratio)
        assert (err <= bound).all(), (what, name, ratio)
        assert not got[sabs == 0].any(), (what, name)                     # no term: exactly zero
    return wt, wp


def _check_grads(p, table, rl, N, q, filter_mode, boundary_mode, g, what):
    """Per element within util.summation_bound of grads64; exact zeros where no term arrives -> (dL/dtable, dL/dxyz)."""
    dt, dp = _bwd(p, table, rl, N, q, filter_mode, boundary_mode, g)
    wt, wp = _check_against(what, dt, dp, p, table, rl, N, q, filter_mode, boundary_mode, g)
    if np.abs(np.asarray(g)).max() > 0:
        assert np.abs(wt).max() > 0, what
    if filter_mode == "nearest":
        assert not wp.any() and not dp.any(), what
    NL, T, _ = np.shape(table)
    assert not dp[ref.empty(p, ref.resolutions(NL, N, q), rl)].any(), what
    return dt, dp


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("F", FS)
def test_forward_and_gradients(F, cfg):
    """filter x boundary x L at this F and table; the source of the coordinates alternates."""
    N, q, NL, T = cfg
    rng = np.random.default_rng(100 + F + N)
    res = ref.resolutions(NL, N, q)
    print(cfg, "resolutions", res, "dense", [ref.is_dense(R, T) for R in res])
    k = F + N
    for filter_mode in ref.FILTERS:
        for boundary_mode in ref.BOUNDARIES:
            for L in LS:
                source = ("lattice", "random")[k % 2]
                k += 1
                rl, p = _coords(source, L)
                table = _table(rng, NL, T, F)
                g = rng.standard_normal(p.shape[:4] + (NL * F,), dtype=f32)
                what = (F, cfg, filter_mode, boundary_mode, L, source)
                out = _check_forward(p, table, rl, N, q, filter_mode, boundary_mode, what)
                if rl is not None:
                    assert not out[rl < 0].any(), what
                _, dp = _check_grads(p, table, rl, N, q, filter_mode, boundary_mode, g, what)
                if filter_mode == "linear" and res[-1] > 1:
                    assert np.abs(dp).max() > 0, what
        k += 1                                                            # (the other source for the other filter at each (boundary, L))
    print("worst err / bound so far", WORST)


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("R", (4, 8, 16))
def test_single_dense_level_is_texture3d(R, F):
    """T = R^3, one level: the same bits as _C.texture_volume_cuda on table[0].reshape(R, R, R, F), forward and dL/dxyz."""
    rl, p = _coords("lattice", 3)
    rng = np.random.default_rng(R + F)
    table = _table(rng, 1, R ** 3, F)
    g = rng.standard_normal(p.shape[:4] + (F,), dtype=f32)
    grid = _cu(table[0].reshape(R, R, R, F))
    for filter_mode in ref.FILTERS:
        for boundary_mode in ref.BOUNDARIES:
            out = _C.hash_grid_cuda(_cu(p), _cu(table), _cu(rl), R, 1.5, filter_mode, boundary_mode)
            vol = _C.texture_volume_cuda(_cu(p), grid, _cu(rl), filter_mode, boundary_mode)
            assert torch.equal(out, vol), (filter_mode, boundary_mode)
            dt, dp = _C.hash_grid_backward_cuda(_cu(p), _cu(table), _cu(rl), R, 1.5, filter_mode, boundary_mode, _cu(g), True, True)
            dg, dv = _C.texture_volume_backward_cuda(_cu(p), grid, _cu(rl), filter_mode, boundary_mode, _cu(g), True, True)
            assert torch.equal(dp, dv), (filter_mode, boundary_mode)
            assert torch.allclose(dt.reshape(dg.shape), dg, rtol=1e-4, atol=1e-4)      # (atomics: the last bits vary; held per element above)


@pytest.mark.parametrize("F", (1, 8))
def test_table_overflow_route(F):
    """One 16 x 16 tile of unrelated positions on a hashed R = 54, T = 4096 level: more than twice as many distinct rows in the
    tile's layer as the scatter's table holds, so most contributions go straight to global memory; next to it a coherent
    surface (a slightly tilted plane across a few voxels) whose rows all find a slot."""
    R, T, shape = 54, 4096, (1, 16, 16, 1)
    assert not ref.is_dense(R, T)
    rng = np.random.default_rng(5)
    scattered = rng.uniform(0, 1, shape + (3,)).astype(f32)
    yy, xx = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    plane = np.stack([0.3 + xx / 16 * 0.1, 0.4 + yy / 16 * 0.1, 0.5 + 0.002 * xx + 0.001 * yy], -1).reshape(shape + (3,)).astype(f32)
    n_scattered = ref.distinct_rows_per_tile(scattered, R, T)
    n_plane = ref.distinct_rows_per_tile(plane, R, T, worst=max)
    print("distinct rows: scattered", n_scattered, "plane", n_plane, "table", table_capacity())
    assert n_scattered > 2 * table_capacity() and 8 < n_plane < table_capacity() // 2
    for p in (scattered, plane):
        table = _table(rng, 1, T, F)
        g = rng.standard_normal(shape + (F,), dtype=f32)
        for boundary_mode in ref.BOUNDARIES:
            _check_forward(p, table, None, R, 24, "linear", boundary_mode, ("overflow", F))
            _check_grads(p, table, None, R, 24, "linear", boundary_mode, g, ("overflow", F, boundary_mode))
        _check_grads(p, table, None, R, 24, "nearest", "clamp", g, ("overflow nearest", F))


@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_empty_slots_next_to_a_poisoned_table(filter_mode, boundary_mode):
    """Negative ids over the zeros shading_vectors writes, NaN, infinities, coordinates beyond the 2^24 rule of the finest level,
    on one axis at a time: zeros out, zero gradient, nothing added to the table.  Two dense levels, 8^3 and 12^3 in 4096 rows;
    the live slots stay in [0.3, 0.9]^3, so nobody reads a voxel of index 0 on any axis, nor a row past R^3: all those hold NaN,
    and an empty slot that sampled voxel (0, 0, 0) would show.  An upstream of all ones deposits one unit per live slot and
    channel into each level."""
    shape, N, q, NL, T, F = (2, 20, 30, 3), 8, 24, 2, 4096, 2
    res = ref.resolutions(NL, N, q)
    assert res == [8, 12] and all(ref.is_dense(R, T) for R in res)
    rng = np.random.default_rng(8)
    p = rng.uniform(0.3, 0.9, shape + (3,)).astype(f32)
    rl = rng.integers(0, 9, shape).astype(np.int32)
    bad = rng.uniform(size=shape) < 0.3
    kind = rng.integers(0, 6, shape)
    rl[bad & (kind == 0)] = -1
    p[bad & (kind == 0)] = (0.0, -0.0, 0.0)
    for k, val in ((1, np.nan), (2, np.inf), (3, -np.inf), (4, 2.0 ** 24 / res[-1] + 1.0), (5, -(2.0 ** 24) / res[-1])):
        p[bad & (kind == k), k % 3] = val
    assert np.array_equal(ref.empty(p, res, rl), bad) and bad.sum() > 300
    table = np.full((NL, T, F), np.nan, f32)
    read = np.zeros((NL, T), bool)
    for l, R in enumerate(res):
        kk, jj, ii = np.meshgrid(np.arange(1, R), np.arange(1, R), np.arange(1, R), indexing="ij")
        read[l, ref.rows(ii, jj, kk, R, T).reshape(-1)] = True
    table[read] = rng.standard_normal((int(read.sum()), F), dtype=f32) + 10
    g = rng.standard_normal(shape + (NL * F,), dtype=f32)
    out = _check_forward(p, table, rl, N, q, filter_mode, boundary_mode, "empty")
    assert (out[bad] == 0).all() and (out[~bad] != 0).all() and np.isfinite(out).all()
    dt, dp = _check_grads(p, table, rl, N, q, filter_mode, boundary_mode, g, "empty")
    assert (dp[bad] == 0).all()
    assert not dt[~read].any()
    dt1, _ = _bwd(p, table, rl, N, q, filter_mode, boundary_mode, np.ones_like(g))
    assert np.allclose(dt1.sum(1), (~bad).sum(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("F", (2, 4, 8))
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_unaligned_and_strided_inputs_give_the_same_bits(F, filter_mode):
    """The table and the upstream gradient as views that start 4 bytes into their storage (no alignment for the F-wide reads),
    and xyz / table / grad_out as non-contiguous views: the same bits as the plain call."""
    N, q, NL, T = 2, 24, 5, 64
    rl, p = _coords("lattice", 3)
    rng = np.random.default_rng(13)
    table = _table(rng, NL, T, F)
    g = rng.standard_normal(p.shape[:4] + (NL * F,), dtype=f32)

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
        modes = (_cu(rl), N, q / 16, filter_mode, boundary_mode)
        out_a = _C.hash_grid_cuda(_cu(p), _cu(table), *modes)
        dt_a, dp_a = _C.hash_grid_backward_cuda(_cu(p), _cu(table), *modes, _cu(g), True, True)
        assert np.array_equal(_bits(_np(out_a)), _bits(ref.forward32(p, table, rl, N, q, filter_mode, boundary_mode)))
        wt, _ = ref.grads64(p, table, rl, N, q, filter_mode, boundary_mode, g)
        st, _ = ref.terms_abs(p, table, rl, N, q, filter_mode, boundary_mode, g)
        for how in (shifted, strided):
            out_u = _C.hash_grid_cuda(how(p) if how is strided else _cu(p), how(table), *modes)
            dt_u, dp_u = _C.hash_grid_backward_cuda(how(p) if how is strided else _cu(p), how(table), *modes, how(g), True, True)
            assert torch.equal(out_a, out_u) and torch.equal(dp_a, dp_u), how.__name__
            assert (np.abs(_np(dt_u) - wt) <= summation_bound(float(np.abs(wt).max()), st)).all(), how.__name__


def test_needs_input_grad_and_repeats():
    """Only what requires grad is computed (one output pointer NULL in the C call), nothing launches when nothing is wanted,
    and dL/dxyz is the same bits on every call and with or without the table's gradient beside it."""
    rl, p = _coords("lattice", 3)
    N, q, NL, T, F = 2, 24, 5, 64, 2
    rng = np.random.default_rng(9)
    table = _table(rng, NL, T, F)
    g = _cu(rng.standard_normal(p.shape[:4] + (NL * F,), dtype=f32))
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    lib = _C.load_library()
    real_b, real_f = lib.dm2_hash_grid_backward, lib.dm2_hash_grid
    calls, fwd_calls = [], []
    words = lambda a: (a[5], a[6]) + a[8:11]                                 # (log2_rows, num_levels, growth16, filter, boundary)

    def spy(*a):
        calls.append((words(a), a[-3].value is not None, a[-2].value is not None))   # (the words, dL_dtable, dL_dxyz not NULL)
        return real_b(*a)

    def spy_f(*a):
        fwd_calls.append(words(a))
        return real_f(*a)
    lib.dm2_hash_grid_backward, lib.dm2_hash_grid = spy, spy_f
    try:
        res = {}
        for need_t, need_p in ((True, True), (True, False), (False, True), (True, True)):
            t, u = _cu(table).requires_grad_(need_t), _cu(p).requires_grad_(need_p)
            out = r.hash_grid(u, t, _cu(rl), N, q / 16, boundary_mode="wrap")
            out.backward(g)
            res.setdefault((need_t, need_p), []).append((t.grad, u.grad))
        code = (6, NL, q, _C.TEX_FILTERS["linear"], _C.TEX_BOUNDARIES["wrap"])
        assert calls == [(code, True, True), (code, True, False), (code, False, True), (code, True, True)]
        assert fwd_calls == [code] * 4
        assert res[(True, False)][0][1] is None and res[(False, True)][0][0] is None
        first, again = res[(True, True)]
        assert torch.equal(first[1], again[1]) and torch.equal(first[1], res[(False, True)][0][1])
        _check_against("table alone", _np(res[(True, False)][0][0]), None, p, table, rl, N, q, "linear", "wrap", _np(g))
        _check_against("xyz alone", None, _np(res[(False, True)][0][1]), p, table, rl, N, q, "linear", "wrap", _np(g))
        del calls[:], fwd_calls[:]
        out = r.hash_grid(_cu(p), _cu(table), _cu(rl), N, q / 16)
        assert out.grad_fn is None and len(fwd_calls) == 1
        w = torch.ones(1, device="cuda", requires_grad=True)
        (out.sum() * w).backward()
        assert _C.hash_grid_backward_cuda(_cu(p), _cu(table), _cu(rl), N, q / 16, "linear", "clamp", g, False, False) == (None, None)
        assert not calls and len(fwd_calls) == 1
    finally:
        lib.dm2_hash_grid_backward, lib.dm2_hash_grid = real_b, real_f


@pytest.mark.parametrize("family", ("all_zero", "one_pixel_per_tile", "one_channel"))
def test_sparse_upstream(family):
    """The slot families of tests/upstream.py hold to the same per-element bound, with exact zeros where no term arrives."""
    N, q, NL, T, F = 2, 24, 5, 64, 4
    rl, p = _coords("lattice", 3)
    table = _table(np.random.default_rng(21), NL, T, F)
    dense = np.random.default_rng(34).standard_normal(p.shape[:4] + (NL * F,)).astype(f32)
    weight = (~ref.empty(p, ref.resolutions(NL, N, q), rl)).sum(-1)
    g, _ = U.mask_slots(family, dense, weight)
    for boundary_mode in ref.BOUNDARIES:
        dt, dp = _check_grads(p, table, rl, N, q, "linear", boundary_mode, g, (family, boundary_mode))
        if family == "all_zero":
            assert not dt.any() and not dp.any()
        else:
            assert np.abs(dt).max() > 0 and np.abs(dp).max() > 0


def test_argument_checks():
    p = torch.full((2, 4, 5, 3, 3), 0.5, device="cuda")
    table = torch.zeros((4, 64, 2), device="cuda")
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32, device="cuda")
    ok = _C.hash_grid_cuda(p, table, rl)
    assert tuple(ok.shape) == (2, 4, 5, 3, 8)
    for args, name in (((p[..., :2], table, rl), "xyz"), ((p.double(), table, rl), "xyz"), ((p, table[:, :48], rl), "table"),
                       ((p, table.half(), rl), "table"), ((p, table, rl[:1]), "render_layers"), ((p, table, rl.long()), "render_layers"),
                       ((p, table, rl, 16, 1.7), "growth")):
        with pytest.raises(RuntimeError, match=name):
            _C.hash_grid_cuda(*args)
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.hash_grid_backward_cuda(p, table, rl, 16, 1.5, "linear", "clamp", ok.double(), True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.hash_grid_cuda(p, table.cpu(), rl)
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    for kw, name in ((dict(filter_mode="cubic"), "filter_mode"), (dict(boundary_mode="mirror"), "boundary_mode"), (dict(growth=1.7), "growth")):
        with pytest.raises(ValueError, match=name):
            r.hash_grid(p, table, rl, **kw)
    for bad_table, name in ((table[:, :48], "T"), (torch.zeros((4, 64, 3), device="cuda"), "F")):
        with pytest.raises(ValueError, match=name):
            r.hash_grid(p, bad_table, rl)
    assert torch.equal(r.hash_grid(p.double(), table, rl.long()), ok)      # (the method converts dtypes, as texture3d does)
    # degenerate sizes: no launch
    for shape in ((0, 4, 5, 2), (2, 4, 5, 0)):
        e = torch.ones(shape + (3,), device="cuda")
        out = _C.hash_grid_cuda(e, table)
        dt, dp = _C.hash_grid_backward_cuda(e, table, None, 16, 1.5, "linear", "clamp", torch.ones_like(out), True, True)
        assert tuple(out.shape) == shape + (8,) and tuple(dt.shape) == tuple(table.shape) and tuple(dp.shape) == shape + (3,) and not dt.any()
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    ptr = lambda t: _C._ptr(t)
    lin, near, CL, WR = _C.TEX_FILTERS["linear"], _C.TEX_FILTERS["nearest"], _C.TEX_BOUNDARIES["clamp"], _C.TEX_BOUNDARIES["wrap"]
    dp = torch.empty_like(p)
    tab, dtab = torch.zeros((2, 4 * 64 * 8), device="cuda")                # room for every accepted call below: F up to 8
    outb, gout = torch.zeros((2, p.shape[:4].numel() * 32), device="cuda")

    def fwd(f=lin, b=CL, N=16, log2T=6, NL=4, F=2, q=24, xyz=p):
        return lib.dm2_hash_grid(2, 4, 5, 3, N, log2T, NL, F, q, f, b, ptr(rl), ptr(xyz) if xyz is not None else None, ptr(tab), ptr(outb), None)

    def bwd(f=lin, b=CL, N=16, log2T=6, NL=4, F=2, q=24, xyz=p):
        return lib.dm2_hash_grid_backward(2, 4, 5, 3, N, log2T, NL, F, q, f, b, ptr(rl), ptr(xyz) if xyz is not None else None,
                                          ptr(tab), ptr(gout), ptr(dtab), ptr(dp), None)
    # ABI 7's word for the same call: a filter of the cube lookup, which knows no such filter any more
    former = 0x800 | (6 << 12) | ((4 - 1) << 17) | ((24 - 17) << 22) | lin | 0x100
    cube = lambda f: lib.dm2_texture_cube(2, 4, 5, 3, 16, 8, 0, f, ptr(rl), ptr(p), ptr(tab), ptr(outb), None)
    cube_b = lambda f: lib.dm2_texture_cube_backward(2, 4, 5, 3, 16, 8, 0, f, ptr(rl), ptr(p), ptr(tab), ptr(gout), ptr(dtab), ptr(dp), None)
    for call, old in ((fwd, cube), (bwd, cube_b)):
        for f, b in ((lin, CL), (lin, WR), (near, CL), (near, WR)):
            assert call(f, b) == 0, (f, b)
        assert call(F=1) == 0 and call(F=4) == 0 and call(F=8) == 0
        assert call(b=2) == 1 and call(b=-1) == 1                          # an unknown boundary
        assert call(F=3) == 1 and call(F=16) == 1 and call(F=0) == 1
        assert call(NL=0) == 1 and call(NL=33) == 1
        assert call(q=16) == 1 and call(q=33) == 1
        assert call(log2T=3) == 1 and call(log2T=25) == 1 and call(log2T=31) == 1
        assert call(N=0) == 1
        assert call(q=32, N=2 ** 18) == 1                                  # R_3 = 2^21
        assert call(q=17, N=2 ** 20 + 1) == 1
        assert call(log2T=24, NL=32, N=1, F=4) == 1                        # NL T F = 2^31
        assert call(xyz=None) == 1                                         # NULL xyz
        for unknown in (2, 4, 0x80, 0x400):
            assert call(f=lin | unknown) == 1, unknown                     # an unknown filter
        assert old(former) == 1 and old(former & ~0x800) == 1 and old(former & ~0x100) == 1, hex(former)
    torch.cuda.synchronize()
    assert not _np(dtab).any() and not _np(outb).any()                    # (a zero table out, g = 0 added)


def _torch_encoding(xyz, table, ids, res):
    """The plain-torch lines hash_grid replaces (linear, clamp)."""
    NL, T, F = table.shape
    outs = []
    for l, R in enumerate(res):
        X = xyz * R - 0.5
        X0 = torch.floor(X)
        f, c0 = X - X0, X0.long()
        c = [[(c0[..., a] + d).clamp(0, R - 1) for d in (0, 1)] for a in range(3)]
        acc = 0
        for k in range(8):
            pp, qq, rr = k & 1, (k >> 1) & 1, (k >> 2) & 1
            i, j, kk = c[0][pp], c[1][qq], c[2][rr]
            row = (kk * R + j) * R + i if R ** 3 <= T else (i ^ (j * 2654435761) ^ (kk * 805459861)) & (T - 1)
            w = (f[..., 0] if pp else 1 - f[..., 0]) * (f[..., 1] if qq else 1 - f[..., 1]) * (f[..., 2] if rr else 1 - f[..., 2])
            acc = acc + w[..., None] * table[l][row]
        outs.append(acc)
    return torch.cat(outs, -1) * (ids >= 0)[..., None]


def test_module_path_end_to_end():
    """rasterize -> shading_vectors -> (position - lo) / (hi - lo) -> hash_grid -> a linear layer (NL F -> 3) -> composite -> a
    random-weighted sum: finite, non-zero table.grad and verts.grad; the encoding bit-equal to forward32; the same image with the
    plain-torch encoding in hash_grid's place within 1e-5 of the maximum."""
    Wm, Hm, bidx, L, N, growth, NL, T, F = 80, 64, [1, 0], 4, 4, 1.5, 6, 512, 2
    res = dm2.Renderer.hash_grid_resolutions(NL, N, growth)
    assert res == ref.resolutions(NL, N, 24) and ref.is_dense(res[1], T) and not ref.is_dense(res[-1], T)
    ts = scenes.tet_lattice(Wm, Hm, 4, seed=scenes.SEED_BASE + 84, num_cams=2).to("cuda")
    r = dm2.LayeredRenderer(ts.mv, ts.proj, Wm, Hm, "cuda")
    assert type(r).hash_grid is dm2.Renderer.hash_grid                   # inherited
    gen = torch.Generator().manual_seed(11)
    table0 = torch.randn((NL, T, F), generator=gen).cuda()
    lin_w = (torch.randn((NL * F, 3), generator=gen) / (NL * F) ** 0.5).cuda()
    alpha0 = torch.rand((ts.faces.shape[0],), generator=gen).cuda() * 0.8 + 0.1
    bg = torch.tensor([0.2, -0.1, 0.5]).cuda()
    verts, table = ts.verts.clone().requires_grad_(True), table0.clone().requires_grad_(True)
    layers, cnt, bary, t = r.rasterize(bidx, verts, ts.faces, L)
    pos = r.shading_vectors(bidx, layers, t)[0]
    lo, hi = ts.verts.min(0).values, ts.verts.max(0).values
    xyz = (pos - lo) / (hi - lo)
    enc = r.hash_grid(xyz, table, layers, N, growth)
    out, acc = r.composite(enc @ lin_w, alpha0, layers, bg)
    wgt = torch.randn(out.shape, generator=gen).cuda()
    (out * wgt).sum().backward()
    assert int(cnt.sum()) > 3000
    for x in (table.grad, verts.grad):
        assert x is not None and torch.isfinite(x).all() and x.abs().max() > 0
    rl, pn = _np(layers), _np(xyz)
    assert np.array_equal(_bits(_np(enc)), _bits(ref.forward32(pn, _np(table0), rl, N, 24, "linear", "clamp")))
    enc_t = _torch_encoding(xyz.detach(), table0, layers, res)
    out_t, _ = r.composite((enc_t @ lin_w).contiguous(), alpha0, layers, bg)
    err = float((out_t - out.detach()).abs().max() / out.detach().abs().max())
    print("composite over the torch encoding against composite over hash_grid", err)
    assert err <= 1e-5
