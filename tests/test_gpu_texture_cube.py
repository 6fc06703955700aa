"""Renderer.texture(boundary_mode="cube") / dm2_texture_cube on the GPU against the contract's restatement
(tests/texture_cube_ref.py): the forward bit-equal to forward32, both gradients within GRAD_TOL of grads64 (per element under
sparse upstream gradients); the two routes of the texel scatter; alignment; needs_input_grad; argument checks; the module
path from rasterize to verts.grad."""
import itertools

import numpy as np
import pytest
import torch

import rasterize_ref as rref
import texture_cube_ref as ref
import texture_ref as ref2d
import upstream as U
from util import GRAD_TOL, rel_linf, scenes, summation_bound, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

CS = (1, 2, 3, 4, 7, 16)
LS = (1, 4)
NS = (1, 2, 5, 64)
SOURCES = rref.SCENES + ("random", "seams")
SHAPE = (2, 40, 50)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _seam_set(N, L):
    """The hand-built set for faces of N texels: the axes, points of the 12 edges and the 8 corners exactly, at lengths 1e-3, 1
    and 1e3, then directions within half a texel of an edge or of a corner from inside every face, at lengths 1e-3 .. 1e3."""
    rng = np.random.default_rng(70 + N)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2] * L
    exact = np.concatenate([ref.exact_directions() * s for s in (1e-3, 1.0, 1e3)])
    m = (n - exact.shape[0] + 1) // 2
    near = ref.near_seams(rng, m, N, reach=0.5)
    near = near / np.linalg.norm(near, axis=-1, keepdims=True) * 10.0 ** rng.uniform(-3, 3, (2 * m, 1))
    d = np.concatenate([exact, near])[:n]
    return rng.permutation(d).reshape(SHAPE + (L, 3)).astype(np.float32)


_DIRS = {}


def _dirs(source, L, N=5):
    """(render_layers or None, dirs) as numpy: the per-vertex random normals of rasterize_ref.scene(source) as rasterize +
    interpolate put them on the frame (-1 ids and zero directions included, lengths as the interpolation leaves them), random
    Gaussian directions without ids, or the hand-built seam set of N."""
    key = (source, L, N if source == "seams" else 0)
    if key not in _DIRS:
        if source == "random":
            _DIRS[key] = (None, np.random.default_rng(40 + L).standard_normal(SHAPE + (L, 3)).astype(np.float32))
        elif source == "seams":
            _DIRS[key] = (None, _seam_set(N, L))
        else:
            s = rref.scene(source)
            layers, cnt, bary, t = _C.rasterize_layers_cuda(s["W"], s["H"], _cu(s["verts"]), _cu(s["faces"]), None, _cu(s["verts_ndc"]),
                                                            _cu(s["verts_image"]), _cu(s["ray_o"]), _cu(s["ray_d"]), L)
            table = np.random.default_rng(50 + L).standard_normal((s["verts"].shape[0], 3)).astype(np.float32)
            d = _C.interpolate_cuda(layers, bary, _cu(table), _cu(s["faces"]))
            _DIRS[key] = (layers.cpu().numpy(), d.cpu().numpy())
    return _DIRS[key]


def _relength(d, seed):
    """The directions at lengths in [0.5, 2] (zero and non-finite ones as they are)."""
    n = np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True)
    ok = np.isfinite(n) & (n > 0)
    want = np.random.default_rng(seed).uniform(0.5, 2.0, n.shape)
    return np.where(ok, d * (want / np.where(ok, n, 1.0)), d).astype(np.float32)


def _tex(rng, B, N, C, per_view):
    return rng.standard_normal(((B,) if per_view else ()) + (6, N, N, C), dtype=np.float32)


def _fwd(d, tex, rl, filter_mode):
    out = _C.texture_cube_cuda(_cu(d), _cu(tex), _cu(rl), filter_mode)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bwd(d, tex, rl, filter_mode, g, need_tex=True, need_dirs=True):
    dt, dd = _C.texture_cube_backward_cuda(_cu(d), _cu(tex), _cu(rl), filter_mode, _cu(g), need_tex, need_dirs)
    torch.cuda.synchronize()
    return (None if dt is None else dt.cpu().numpy()), (None if dd is None else dd.cpu().numpy())


def _check_forward(d, tex, rl, filter_mode, what):
    got = _fwd(d, tex, rl, filter_mode)
    want = ref.forward32(d, tex, rl, filter_mode)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
    return got


def _check_grads(d, tex, rl, filter_mode, g, what):
    dt, dd = _bwd(d, tex, rl, filter_mode, g)
    wt, wd = ref.grads64(d, tex, rl, filter_mode, g)
    assert dt.shape == tex.shape and dd.shape == d.shape, what
    et, ed = rel_linf(dt, wt), rel_linf(dd, wd)
    print(what, "dtex", et, "ddir", ed)
    assert np.abs(wt).max() > 0, what
    assert np.isfinite(dt).all() and et <= GRAD_TOL, (what, "dtex", et)
    if filter_mode == "nearest":
        assert not wd.any() and not dd.any(), what
    else:
        assert np.abs(wd).max() > 0, what
        assert np.isfinite(dd).all() and ed <= GRAD_TOL, (what, "ddir", ed)
    assert (dd[ref.empty(d, rl)] == 0).all(), what
    return dt, dd


def _assert_covers(st, N, what, borders=False):
    """From the reference's stage: every face, seam taps and corner samples occur (on large faces a frame of random directions
    holds a handful of corner samples at most: there only the hand-built set is held to it); ``borders``: a seam tap across
    each of the 24 (face, border) pairs and a corner sample at each of the 24 (face, corner) pairs."""
    live = ~st["empty"]
    assert set(np.unique(st["face"][live]).tolist()) == set(range(6)), what
    assert (st["seam"].any(-1) & live).sum() > 50, what
    if N <= 5 or borders:
        assert ((st["miss"] >= 0) & live).sum() > 50, what
    if borders:
        lo_x, hi_x, lo_y, hi_y = st["i0"] == -1, st["i0"] == N - 1, st["j0"] == -1, st["j0"] == N - 1
        for f in range(6):
            on = live & (st["face"] == f)
            for k, b in enumerate((lo_x, hi_x, lo_y, hi_y)):
                assert (on & b).any(), (what, "face", f, "border", k)
            for bx, by in itertools.product((lo_x, hi_x), (lo_y, hi_y)):
                assert (on & bx & by & (st["miss"] >= 0)).any(), (what, "face", f, "a corner")


def _forward_grid(N, per_view, Cs, Ls, sources):
    rng = np.random.default_rng(100 + N)
    big = _tex(rng, 3, N, max(Cs), per_view)
    big_gpu = _cu(big)
    stages = {}
    for C in Cs:
        tex_c, tex_c_gpu = np.ascontiguousarray(big[..., :C]), big_gpu[..., :C].contiguous()
        for L, source in itertools.product(Ls, sources):
            rl, d = _dirs(source, L, N)
            B = d.shape[0]
            tex, tex_gpu = (tex_c[:B], tex_c_gpu[:B]) if per_view else (tex_c, tex_c_gpu)
            d_gpu, rl_gpu = _cu(d), _cu(rl)
            for filter_mode in ref.FILTERS:
                key = (L, source, filter_mode)
                if key not in stages:
                    stages[key] = st = ref.stage(d, N, rl, filter_mode)
                    if filter_mode == "linear" and L == 4 and (source == "seams" or (N <= 64 and source in ("random", "soup"))):
                        _assert_covers(st, N, (N, source), borders=source == "seams")
                got = _C.texture_cube_cuda(d_gpu, tex_gpu, rl_gpu, filter_mode).cpu().numpy()
                want = ref.blend(stages[key], tex, filter_mode)
                what = (N, per_view, L, source, C, filter_mode)
                assert got.shape == d.shape[:4] + (C,) and got.dtype == np.float32, what
                assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
                filled = int((~stages[key]["empty"]).sum())
                if source == "no_faces":
                    assert (got == 0).all() and filled == 0
                else:
                    assert 0.99 * filled <= (np.abs(got).max(-1) > 0).sum() <= filled and filled > 0, what


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("N", NS)
def test_forward_bit_equal_to_restatement(N, per_view):
    """Both filters x CS x LS x SOURCES at this face size and sharing."""
    _forward_grid(N, per_view, CS, LS, SOURCES)


def test_forward_bit_equal_n512():
    _forward_grid(512, False, (3, 16), (4,), ("random", "seams", "lattice"))


# (C, per_view, L, N, source): every value of each axis appears, with both filters
GRAD_GRID = [(1, False, 1, 1, "random"), (2, True, 4, 2, "seams"), (3, False, 4, 5, "soup"), (4, True, 1, 64, "seams"),
             (7, False, 4, 64, "lattice"), (16, True, 4, 5, "random"), (16, False, 1, 2, "seams"), (3, True, 4, 1, "seams"),
             (4, False, 4, 5, "seams"), (1, True, 1, 64, "random"), (2, False, 4, 1, "lattice"), (7, True, 1, 2, "soup")]


def test_gradient_grid_covers_every_axis():
    seen = [set(x) for x in zip(*GRAD_GRID)]
    assert seen == [set(CS), {False, True}, set(LS), set(NS), {"random", "seams", "soup", "lattice"}]


@pytest.mark.parametrize("k", range(len(GRAD_GRID)))
def test_gradients_against_float64(k):
    C, per_view, L, N, source = GRAD_GRID[k]
    rl, d = _dirs(source, L, N)
    d = _relength(d, 300 + k)
    rng = np.random.default_rng(200 + k)
    tex = _tex(rng, d.shape[0], N, C, per_view)
    g = rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32)
    if source == "seams":
        _assert_covers(ref.stage(d, N, rl, "linear"), N, GRAD_GRID[k], borders=True)
    for filter_mode in ref.FILTERS:
        _check_forward(d, tex, rl, filter_mode, (k, filter_mode))
        _check_grads(d, tex, rl, filter_mode, g, GRAD_GRID[k] + (filter_mode,))


@pytest.mark.parametrize("C", ref2d.INST_CS)
def test_every_instantiation_once(C):
    """Both filters x N = 2 and 5 x shared and per-view cubes at this C on texture_cube_ref.instantiation_case() (the gradient
    grid above is thinned): every instantiation of the three kernels that C selects, at the smallest shape with two views,
    partial tiles, two layers, empty slots in every tile, seam taps across every border and corner samples."""
    rng = np.random.default_rng(900 + C)
    for N in ref.INST_NS:
        d, rl = ref.instantiation_case(N)
        bad = ref.empty(d, rl)
        g = rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32)
        for per_view in (False, True):
            tex = _tex(rng, d.shape[0], N, C, per_view)
            for filter_mode in ref.FILTERS:
                what = ("instantiation", C, N, per_view, filter_mode)
                out = _check_forward(d, tex, rl, filter_mode, what)
                assert (out[bad] == 0).all(), what
                _check_grads(d, tex, rl, filter_mode, g, what)


SPARSE = [("lattice", 4, 5, True), ("seams", 1, 2, False), ("random", 4, 64, False)]


@pytest.mark.parametrize("source,L,N,per_view", SPARSE, ids=[f"{s}-L{L}-N{N}" for s, L, N, _ in SPARSE])
def test_sparse_upstream(source, L, N, per_view):
    """The slot families of tests/upstream.py; per element |got - float64| <= GRAD_TOL max|float64| + 8 eps32 sum|terms|
    (util.summation_bound), and exactly zero where no term arrives.  The terms of dL/dtex are the w_k g of the slots that
    address the texel; those of dL/ddir[s, k] the channels' g[s, c] d out[s, c] / d dir[s, k]."""
    C = 3
    rl, d = _dirs(source, L, N)
    d = _relength(d, 500 + N)
    tex = _tex(np.random.default_rng(400 + L), d.shape[0], N, C, per_view)
    dense = np.random.default_rng(34 + L).standard_normal(d.shape[:4] + (C,)).astype(np.float32)
    empty = ref.empty(d, rl)
    weight = (~empty).sum(-1)
    jac = []                                                              # d out[s, c] / d dir[s, :], one channel at a time
    for c in range(C):
        one = np.zeros(dense.shape)
        one[..., c] = 1.0
        jac.append(ref.grads64(d, tex, rl, "linear", one)[1])
    for family in U.slot_families(dense):
        g, _ = U.mask_slots(family, dense, weight)
        dt, dd = _bwd(d, tex, rl, "linear", g)
        assert np.isfinite(dt).all() and np.isfinite(dd).all()
        if family == "all_zero":
            assert not dt.any() and not dd.any()
            continue
        wt, wd = ref.grads64(d, tex, rl, "linear", g)
        assert np.abs(wt).max() > 0 and np.abs(wd).max() > 0, family
        st = ref.tex_terms_abs(d, tex, rl, "linear", g)
        sd = sum(np.abs(g[..., c, None].astype(np.float64)) * np.abs(jac[c]) for c in range(C))
        for name, got, want, sabs in (("tex", dt, wt, st), ("dir", dd, wd, sd)):
            err, bound = np.abs(got - want), summation_bound(float(np.abs(want).max()), sabs)
            print(source, family, name, "worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (source, family, name, float((err / bound).max()))
            assert not got[sabs == 0].any(), (source, family, name)       # no term: exactly zero
        live = ~empty & (g != 0).any(-1)
        assert not dd[~live].any(), (source, family)


@pytest.mark.parametrize("C", [3, 16])
def test_table_overflow_route(C):
    """Random directions on faces of 64^2: every 16 x 16 tile addresses about 1000 distinct texels per layer, twice what the
    scatter's LDS table holds; the texels that find no slot add straight to global memory."""
    N, shape = 64, (2, 48, 64, 4)
    rng = np.random.default_rng(5)
    d = rng.standard_normal(shape + (3,)).astype(np.float32)
    least = ref.distinct_texels_per_tile(d, N, None, "linear")
    print("distinct texels per tile and layer, at least", least)
    assert least > table_capacity()
    rl = rng.integers(-1, 6, shape).astype(np.int32)
    for per_view in (False, True):
        tex = _tex(rng, shape[0], N, C, per_view)
        g = rng.standard_normal(shape + (C,), dtype=np.float32)
        for layers in (None, rl):
            _check_forward(d, tex, layers, "linear", ("overflow", C, per_view))
            _check_grads(d, tex, layers, "linear", g, ("overflow", C, per_view, layers is not None))
        _check_grads(d, tex, None, "nearest", g, ("overflow nearest", C, per_view))


@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_every_lane_on_one_cube_corner(C, filter_mode):
    """Every slot within a fifth of a texel of the corner (+1, +1, +1), from all three faces: three texels per tile (one per
    lane for nearest, one of the three), every sample a three-tap sample."""
    N, shape = 5, (2, 50, 70, 4)
    rng = np.random.default_rng(6)
    d = (1.0 - rng.uniform(0.0, 0.2 * 2 / N, shape + (3,))).astype(np.float32)
    d[..., 0] = np.where(rng.integers(0, 3, shape) == 0, 1.0, d[..., 0])  # (so that each face is the major one somewhere)
    st = ref.stage(d, N, None, "linear")
    assert (st["miss"] >= 0).all() and set(np.unique(st["face"]).tolist()) == {0, 2, 4}
    most = ref.distinct_texels_per_tile(d, N, None, filter_mode, worst=max)
    assert most == 3
    for per_view in (False, True):
        tex = _tex(rng, shape[0], N, C, per_view)
        g = rng.standard_normal(shape + (C,), dtype=np.float32)
        _check_forward(d, tex, None, filter_mode, ("corner", C, per_view))
        dt, _ = _check_grads(d, tex, None, filter_mode, g, ("corner", C, per_view))
        assert ((dt != 0).any(-1).reshape(-1, 6 * N * N).sum(-1) == 3).all()


def test_empty_slots():
    """Negative ids, NaN / inf / all-zero (of either sign) directions: zeros out, zero gradient, nothing added to the cube."""
    shape, N, C = (2, 20, 30, 3), 4, 3
    rng = np.random.default_rng(8)
    d = rng.standard_normal(shape + (3,)).astype(np.float32)
    rl = rng.integers(0, 9, shape).astype(np.int32)
    bad = rng.uniform(size=shape) < 0.3
    kind = rng.integers(0, 6, shape)
    rl[bad & (kind == 0)] = -1
    for k, val in ((1, np.nan), (2, np.inf), (3, -np.inf)):
        d[bad & (kind == k), k % 3] = val
    d[bad & (kind == 4)] = 0.0
    d[bad & (kind == 5)] = (-0.0, 0.0, -0.0)
    assert np.array_equal(ref.empty(d, rl), bad) and bad.sum() > 300
    tex = _tex(rng, shape[0], N, C, False) + 10
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    for filter_mode in ref.FILTERS:
        out = _check_forward(d, tex, rl, filter_mode, "empty")
        assert (out[bad] == 0).all() and (out[~bad] != 0).all()
        dt, dd = _check_grads(d, tex, rl, filter_mode, g, "empty")
        assert (dd[bad] == 0).all()
        # all-ones upstream: the cube receives exactly one unit of weight per live slot and channel
        dt1, _ = _bwd(d, tex, rl, filter_mode, np.ones_like(g))
        assert np.allclose(dt1.sum((0, 1, 2)), (~bad).sum(), rtol=1e-5, atol=0)


def test_needs_input_grad():
    rl, d = _dirs("lattice", 4)
    C, N = 6, 5
    rng = np.random.default_rng(9)
    tex = _tex(rng, 1, N, C, False)
    g = _cu(rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32))
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    calls = []
    real = _C.texture_cube_backward_cuda

    def spy(*a):
        calls.append(tuple(a[-2:]))
        return real(*a)
    _C.texture_cube_backward_cuda = spy
    try:
        res = {}
        for need_t, need_d in ((True, True), (True, False), (False, True)):
            t, u = _cu(tex).requires_grad_(need_t), _cu(d).requires_grad_(need_d)
            out = r.texture(u, t, _cu(rl), boundary_mode="cube")
            out.backward(g)
            res[(need_t, need_d)] = (None if t.grad is None else t.grad.clone(), None if u.grad is None else u.grad.clone())
        assert calls == [(True, True), (True, False), (False, True)]
        assert res[(True, False)][1] is None and res[(False, True)][0] is None
        # dL/ddir is a pure function of the inputs: the same bits with and without the cube's gradient
        assert torch.equal(res[(True, True)][1], res[(False, True)][1])
        assert rel_linf(res[(True, False)][0].cpu().numpy(), res[(True, True)][0].cpu().numpy()) <= GRAD_TOL
        wt, wd = ref.grads64(d, tex, rl, "linear", g.cpu().numpy())
        assert np.abs(wt).max() > 0 and np.abs(wd).max() > 0
        assert rel_linf(res[(True, False)][0].cpu().numpy(), wt) <= GRAD_TOL
        assert rel_linf(res[(False, True)][1].cpu().numpy(), wd) <= GRAD_TOL
        del calls[:]
        launches = []
        lib = _C.load_library()
        real_b = lib.dm2_texture_cube_backward
        lib.dm2_texture_cube_backward = lambda *a: launches.append("b") or real_b(*a)
        try:
            out = r.texture(_cu(d), _cu(tex), _cu(rl), boundary_mode="cube")
            assert out.grad_fn is None
            w = torch.ones(1, device="cuda", requires_grad=True)
            (out.sum() * w).backward()
            assert real(_cu(d), _cu(tex), _cu(rl), "linear", g, False, False) == (None, None)
            # one output wanted: one kernel's pointer is NULL in the C call
            real(_cu(d), _cu(tex), _cu(rl), "linear", g, True, False)
            real(_cu(d), _cu(tex), _cu(rl), "linear", g, False, True)
        finally:
            lib.dm2_texture_cube_backward = real_b
        assert not calls and launches == ["b", "b"]
    finally:
        _C.texture_cube_backward_cuda = real


@pytest.mark.parametrize("C", [4, 16])
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_unaligned_tables_give_the_same_bits(C, filter_mode):
    """tex and the upstream gradient as views that start 4 bytes into their storage (no 16-byte alignment): the four-channel
    reads do not apply; the results are the same bits as with aligned tensors."""
    N = 5
    rl, d = _dirs("seams", 4, N)
    rng = np.random.default_rng(13)
    tex = _tex(rng, 1, N, C, False)
    g = rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = _cu(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    args, modes = (_cu(d),), (None, filter_mode)
    out_a = _C.texture_cube_cuda(*args, _cu(tex), *modes)
    out_u = _C.texture_cube_cuda(*args, shifted(tex), *modes)
    dt_a, dd_a = _C.texture_cube_backward_cuda(*args, _cu(tex), *modes, _cu(g), True, True)
    dt_u, dd_u = _C.texture_cube_backward_cuda(*args, shifted(tex), *modes, shifted(g), True, True)
    assert torch.equal(out_a, out_u) and torch.equal(dd_a, dd_u)
    assert np.array_equal(_bits(out_u.cpu().numpy()), _bits(ref.forward32(d, tex, None, filter_mode)))
    assert rel_linf(dt_u.cpu().numpy(), dt_a.cpu().numpy()) <= GRAD_TOL
    wt, wd = ref.grads64(d, tex, None, filter_mode, g)
    assert rel_linf(dt_u.cpu().numpy(), wt) <= GRAD_TOL and rel_linf(dd_u.cpu().numpy(), wd) <= GRAD_TOL


def test_argument_checks():
    d = torch.ones((2, 4, 5, 3, 3), device="cuda")
    tex = torch.zeros((6, 8, 8, 3), device="cuda")
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32, device="cuda")
    ok = _C.texture_cube_cuda(d, tex, rl)
    assert tuple(ok.shape) == (2, 4, 5, 3, 3)
    for args, name in (((d[..., :2], tex, rl), "dirs"), ((d[0], tex, rl[0]), "dirs"), ((d.double(), tex, rl), "dirs"),
                       ((d, tex[0], rl), "tex"), ((d, tex[None].expand(3, 6, 8, 8, 3), rl), "tex"), ((d, tex[:5], rl), "tex"),
                       ((d, tex[:, :7], rl), "tex"), ((d, tex[:, :, :7], rl), "tex"), ((d, tex[:, :0, :0], rl), "tex"),
                       ((d, tex[..., :0], rl), "tex"), ((d, tex.half(), rl), "tex"),
                       ((d, tex, rl[:1]), "render_layers"), ((d, tex, rl.long()), "render_layers")):
        with pytest.raises(RuntimeError, match=name):
            _C.texture_cube_cuda(*args)
    with pytest.raises(RuntimeError, match="filter_mode"):
        _C.texture_cube_cuda(d, tex, rl, "cubic")
    with pytest.raises(RuntimeError, match="filter_mode"):
        _C.texture_cube_cuda(d, tex, rl, "linear-mipmap-linear")
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.texture_cube_backward_cuda(d, tex, rl, "linear", ok[..., :2], True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_cube_cuda(d.cpu(), tex.cpu(), rl.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_cube_cuda(d, tex.cpu(), rl)
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    uv_da = torch.zeros((2, 4, 5, 3, 4), device="cuda")
    for kw in (dict(filter_mode="linear-mipmap-linear"), dict(filter_mode="linear-mipmap-linear", uv_da=uv_da), dict(uv_da=uv_da),
               dict(mip=torch.zeros((10, 3), device="cuda")), dict(max_mip_level=2)):
        with pytest.raises(ValueError, match="boundary_mode"):
            r.texture(d, tex, rl, boundary_mode="cube", **kw)
    with pytest.raises(RuntimeError, match="filter_mode"):
        r.texture(d, tex, rl, filter_mode="trilinear", boundary_mode="cube")
    # _C.texture_cuda itself does not know the mode: the method dispatches before reaching it
    with pytest.raises(RuntimeError, match="boundary_mode"):
        _C.texture_cuda(d[..., :2], tex[0], rl, "linear", "cube")
    assert torch.equal(r.texture(d, tex, rl, boundary_mode="cube"), ok)
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    p = lambda t: _C._ptr(t)
    assert lib.dm2_texture_cube(2, 4, 5, 3, 8, 3, 0, 1, p(rl), p(d), p(tex), p(ok), None) == 0
    assert lib.dm2_texture_cube(2, 4, 5, 3, 0, 3, 0, 1, p(rl), p(d), p(tex), p(ok), None) == 1
    assert lib.dm2_texture_cube(2, 4, 5, 3, 18919, 3, 0, 1, p(rl), p(d), p(tex), p(ok), None) == 1
    assert lib.dm2_texture_cube(2, 4, 5, 3, 8, 3, 0, 1, p(rl), None, p(tex), p(ok), None) == 1
    assert lib.dm2_texture_cube(2, 4, 5, 3, 8, 3, 0, 2, p(rl), p(d), p(tex), p(ok), None) == 1
    assert lib.dm2_texture_cube(2, 4, 5, 3, 8, 0, 0, 1, p(rl), p(d), p(tex), p(ok), None) == 1
    assert lib.dm2_texture_cube_backward(2, 4, 5, 3, 0, 3, 0, 1, p(rl), p(d), p(tex), p(ok), p(tex), p(d), None) == 1
    assert lib.dm2_texture_cube_backward(2, 4, 5, 3, 18919, 3, 0, 1, p(rl), p(d), p(tex), p(ok), p(tex), p(d), None) == 1
    assert lib.dm2_texture_cube_backward(2, 4, 5, 3, 8, 3, 0, 1, p(rl), None, p(tex), p(ok), p(tex), p(d), None) == 1
    torch.cuda.synchronize()


def test_degenerate_sizes():
    tex = _cu(_tex(np.random.default_rng(10), 1, 4, 3, False))
    launches = []
    lib = _C.load_library()
    real_f, real_b = lib.dm2_texture_cube, lib.dm2_texture_cube_backward
    try:
        lib.dm2_texture_cube = lambda *a: launches.append("f") or real_f(*a)
        lib.dm2_texture_cube_backward = lambda *a: launches.append("b") or real_b(*a)
        for shape in ((0, 4, 5, 2), (2, 0, 5, 2), (2, 4, 0, 2), (2, 4, 5, 0)):
            d = torch.ones(shape + (3,), device="cuda")
            rl = torch.zeros(shape, dtype=torch.int32, device="cuda")
            for layers in (None, rl):
                out = _C.texture_cube_cuda(d, tex, layers)
                assert tuple(out.shape) == shape + (3,) and out.dtype == torch.float32
                dt, dd = _C.texture_cube_backward_cuda(d, tex, layers, "linear", torch.ones_like(out), True, True)
                assert tuple(dt.shape) == tuple(tex.shape) and tuple(dd.shape) == shape + (3,) and (dt == 0).all()
        assert not launches
    finally:
        lib.dm2_texture_cube, lib.dm2_texture_cube_backward = real_f, real_b


@pytest.mark.parametrize("name", ["lattice", "soup"])
def test_module_path_end_to_end(name):
    """rasterize -> interpolate (per-vertex normals) -> torch normalize -> texture(boundary_mode="cube") -> composite -> a
    random-weighted sum: finite, non-zero tex.grad and verts.grad; tex.grad against the _C calls composed by hand and against
    grads64 fed the composite's gradient."""
    assert "TextureCubeFunction" in dm2.__all__ and issubclass(dm2.TextureCubeFunction, torch.autograd.Function)
    W, H, bidx, L, C, N = 80, 64, [1, 0], 4, 3, 16
    if name == "lattice":
        ts = scenes.tet_lattice(W, H, 4, seed=scenes.SEED_BASE + 84, num_cams=2).to("cuda")
    else:
        ts = scenes.triangle_soup(W, H, 600, scenes.SEED_BASE + 85, num_cams=2, depth_complexity=12.0, shared_verts=True).to("cuda")
    mv, proj, verts0, faces = ts.mv, ts.proj, ts.verts, ts.faces
    r = dm2.LayeredRenderer(mv, proj, W, H, "cuda")
    assert type(r).texture is dm2.Renderer.texture                       # inherited
    gen = torch.Generator().manual_seed(11)
    normals0 = torch.randn((verts0.shape[0], 3), generator=gen).cuda()
    tex0 = torch.randn((6, N, N, C), generator=gen).cuda()
    alpha0 = torch.rand((faces.shape[0],), generator=gen).cuda() * 0.8 + 0.1
    bg = torch.tensor([0.2, -0.1, 0.5]).cuda()
    verts, normals, tex = (x.clone().requires_grad_(True) for x in (verts0, normals0, tex0))
    layers, cnt, bary, t = r.rasterize(bidx, verts, faces, L)
    nrm = r.interpolate(layers, bary, normals, faces)
    dirs = torch.nn.functional.normalize(nrm, dim=-1)
    shaded = r.texture(dirs, tex, layers, boundary_mode="cube")
    out, acc = r.composite(shaded, alpha0, layers, bg)
    wgt = torch.randn(out.shape, generator=gen).cuda()
    (out * wgt).sum().backward()
    assert int(cnt.sum()) > 3000
    for x in (tex.grad, verts.grad, normals.grad):
        assert x is not None and torch.isfinite(x).all() and x.abs().max() > 0
    rl, dn, tn = (x.detach().cpu().numpy() for x in (layers, dirs, tex0))
    assert np.array_equal(_bits(shaded.detach().cpu().numpy()), _bits(ref.forward32(dn, tn, rl, "linear")))
    # by hand: the composite's backward, then the cube's
    _, _, _, n_contrib = _C.composite_cuda(shaded.detach(), alpha0, layers, bg)
    dvalues, _ = _C.composite_backward_cuda(shaded.detach(), alpha0, layers, bg, n_contrib, wgt, None, True, False)
    dtex, ddir = _C.texture_cube_backward_cuda(dirs.detach(), tex0, layers, "linear", dvalues, True, True)
    torch.cuda.synchronize()
    e_hand = rel_linf(tex.grad.cpu().numpy(), dtex.cpu().numpy())
    wt, wd = ref.grads64(dn, tn, rl, "linear", dvalues.cpu().numpy())
    e_ref, e_dir = rel_linf(tex.grad.cpu().numpy(), wt), rel_linf(ddir.cpu().numpy(), wd)
    print(name, "tex.grad against the hand-composed calls", e_hand, "against grads64", e_ref, "ddir", e_dir)
    assert np.abs(wt).max() > 0 and np.abs(wd).max() > 0
    assert e_hand <= GRAD_TOL and e_ref <= GRAD_TOL and e_dir <= GRAD_TOL
