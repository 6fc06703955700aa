"""Renderer.texture(filter_mode="linear-mipmap-linear", boundary_mode="cube", mip_level=...) / dm2_texture_cube_mip
on the GPU against the contract's restatement (tests/texture_cube_mip_ref.py): the forward bit-equal to
forward32; dL/dtex, dL/dmip and dL/ddirs within GRAD_TOL of grads64, dL/dmip_level per element; the level's branch points; seams
and corners at every level size; both routes of the texel scatter; alignment; needs_input_grad; argument checks down to the C
ABI; the module path from rasterize to the gradients of a per-face roughness, of the cube and of the vertices."""
import itertools

import numpy as np
import pytest
import torch

import composite_ref
import interpolate_ref
import normals_ref
import rasterize_ref as rref
import shading_ref
import texture_cube_mip_ref as ref
import texture_cube_ref as cref
import texture_mip_ref as mref
import upstream as U
from util import EPS32, GRAD_TOL, rel_linf, scenes, summation_bound, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

CS = (1, 2, 3, 4, 7, 16)
LS = (1, 4)
NS = (1, 2, 4, 5, 6, 8)                        # chains of 1, 2, 3, 1, 2 and 4 levels
MAX_LEVELS = (None, 0, 1)
SHAPE = (2, 20, 27)                            # two views, partial tiles


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _inputs(N, L, seed, max_mip_level=None, shape=SHAPE):
    """dirs: random ones, a third of them near the seams of one of the level sizes, a few empty (NaN, zero); levels in
    [-1, nlev + 1], a few not finite; ids with -1 in one slot of eight."""
    rng = np.random.default_rng(seed)
    nlev = ref.layout(N, max_mip_level)[0]
    n = int(np.prod(shape)) * L
    d = rng.standard_normal((n, 3)) * np.exp(rng.uniform(-2, 2, (n, 1)))
    for k in range(nlev):
        aimed = cref.near_seams(rng, n // (6 * nlev), N >> k)
        d[rng.choice(n, len(aimed), replace=False)] = aimed
    d = d.reshape(shape + (L, 3)).astype(np.float32)
    lod = rng.uniform(-1, nlev + 1, shape + (L,)).astype(np.float32)
    bad = rng.uniform(size=shape + (L,))
    d[bad < 0.01, 1] = np.nan
    d[(bad >= 0.01) & (bad < 0.02)] = 0.0
    lod[(bad >= 0.02) & (bad < 0.03)] = np.nan
    lod[(bad >= 0.03) & (bad < 0.04)] = np.inf
    rl = np.where(rng.uniform(size=shape + (L,)) < 1 / 8, -1, rng.integers(0, 50, shape + (L,))).astype(np.int32)
    return d, lod, rl


def _cube(rng, B, N, C, per_view, max_mip_level=None, box=False):
    tex = rng.standard_normal(((B,) if per_view else ()) + (6, N, N, C), dtype=np.float32)
    T = ref.layout(N, max_mip_level)[2]
    mip = ref.box_chain(tex, max_mip_level) if box else rng.standard_normal(tex.shape[:-3] + (T, C), dtype=np.float32)
    return tex, mip


def _fwd(d, lod, tex, mip, rl, max_mip_level=None):
    out = _C.texture_cube_mip_cuda(_cu(d), _cu(lod), _cu(tex), _cu(mip), _cu(rl), max_mip_level)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bwd(d, lod, tex, mip, rl, max_mip_level, g, needs=(True, True, True, True)):
    res = _C.texture_cube_mip_backward_cuda(_cu(d), _cu(lod), _cu(tex), _cu(mip), _cu(rl), max_mip_level, _cu(g), *needs)
    torch.cuda.synchronize()
    return tuple(_np(x) for x in res)


def _check_forward(d, lod, tex, mip, rl, max_mip_level, what):
    got = _fwd(d, lod, tex, mip, rl, max_mip_level)
    want = ref.forward32(d, lod, tex, mip, rl, max_mip_level)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
    return got


def _level_bound(wl, terms):
    """dL/dmip_level is a difference of two samples: 1e-5 max|g64| + 8 eps32 sum_c |g_c| (|c_j| + |c_{j+1}|), util.summation_bound's
    form with the terms of that difference."""
    return 1e-5 * float(np.abs(wl).max()) + 8.0 * EPS32 * terms


def _check_grads(d, lod, tex, mip, rl, max_mip_level, g, what):
    dt, dm, dd, dl = _bwd(d, lod, tex, mip, rl, max_mip_level, g)
    wt, wm, wd, wl, terms = ref.grads64(d, lod, tex, mip, rl, max_mip_level, g)
    assert dt.shape == tex.shape and dm.shape == mip.shape and dd.shape == d.shape and dl.shape == lod.shape, what
    errs = {}
    for name, got, want in (("dtex", dt, wt), ("dmip", dm, wm), ("ddir", dd, wd)):
        assert np.isfinite(got).all(), (what, name)
        if not want.any():                                                # a gradient whose reference is all zeros is exactly zero
            assert not got.any(), (what, name)
            continue
        errs[name] = rel_linf(got, want)
        assert errs[name] <= GRAD_TOL, (what, name, errs[name])
    assert wt.any() or wm.any(), what
    assert np.isfinite(dl).all(), what
    if not wl.any():
        assert not dl.any(), what
    else:
        err, bound = np.abs(dl - wl), _level_bound(wl, terms)
        errs["dlevel / bound"] = float((err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), (what, "dlevel", errs["dlevel / bound"])
        assert not dl[terms == 0].any(), what                             # clamped or empty: exactly zero
    print(what, errs)
    empty = ref.stage(d, lod, tex.shape[-2], rl, max_mip_level)["empty"]
    assert (dd[empty] == 0).all() and (dl[empty] == 0).all(), what
    return dt, dm, dd, dl


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("N", NS)
def test_forward_bit_equal_to_restatement(N, per_view):
    """CS x LS x MAX_LEVELS at this face size and sharing, random levels in [-1, nlev + 1], a chain that is not the box chain."""
    rng = np.random.default_rng(100 + N)
    for max_mip_level, L in itertools.product(MAX_LEVELS, LS):
        d, lod, rl = _inputs(N, L, 10 * N + L, max_mip_level)
        big, bigm = _cube(rng, SHAPE[0], N, max(CS), per_view, max_mip_level)
        st = ref.stage(d, lod, N, rl, max_mip_level)
        nlev = st["nlev"]
        assert nlev == {None: {1: 1, 2: 2, 4: 3, 5: 1, 6: 2, 8: 4}[N], 0: 1, 1: min(2, 1 + (N % 2 == 0))}[max_mip_level]
        live = ~st["empty"]
        assert (live & (st["lod"] <= 0)).sum() > 20 and (live & (st["lod"] >= nlev - 1)).sum() > 20 and st["empty"].sum() > 20
        for k in range(nlev - 1):
            assert (st["two"] & (st["j"] == k)).sum() > 20, (N, max_mip_level, k)
        for C in CS:
            tex, mip = np.ascontiguousarray(big[..., :C]), np.ascontiguousarray(bigm[..., :C])
            got = _check_forward(d, lod, tex, mip, rl, max_mip_level, (N, per_view, max_mip_level, L, C))
            assert (got[st["empty"]] == 0).all()
            assert (np.abs(got).max(-1) > 0).sum() == live.sum()
        _check_forward(d, lod, tex, mip, None, max_mip_level, (N, per_view, max_mip_level, L, "no ids"))


@pytest.mark.parametrize("N,max_mip_level", [(4, None), (8, None), (8, 1), (5, None)])
def test_level_edge_set(N, max_mip_level):
    """Every integer level 0 .. nlev and the floats next to each, +-0, a denormal, +-1e30; NaN and +-inf give empty slots.  At
    or below 0 the bits are the cube op's "linear"; the level's gradient is zero at and beyond the ends and the right-hand
    derivative at an integer inside."""
    nlev = ref.layout(N, max_mip_level)[0]
    edges = ref.level_edges(nlev)
    rng = np.random.default_rng(20 + N)
    shape, C = (1, 16, 24, 2), 3
    d, _, rl = _inputs(N, 2, 21, max_mip_level, shape[:3])
    lod = edges[np.arange(int(np.prod(shape))) % len(edges)].reshape(shape)
    tex, mip = _cube(rng, 1, N, C, False, max_mip_level)
    got = _check_forward(d, lod, tex, mip, rl, max_mip_level, ("edges", N))
    low = (lod <= 0) & np.isfinite(lod)                                   # (-inf: an empty slot here, not in the cube op)
    assert low.sum() > 100 and np.array_equal(_bits(got[low]), _bits(_np(_C.texture_cube_cuda(_cu(d), _cu(tex), _cu(rl), "linear"))[low]))
    assert (got[~np.isfinite(lod)] == 0).all()
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    *_, dl = _check_grads(d, lod, tex, mip, rl, max_mip_level, g, ("edges", N, max_mip_level))
    clamped = (lod <= 0) | (lod >= nlev - 1) | ~np.isfinite(lod)
    assert not dl[clamped].any()
    if nlev > 2:
        inside = (lod == 1) & (rl >= 0) & np.isfinite(d).all(-1) & (d != 0).any(-1)
        assert inside.sum() > 5 and (dl[inside] != 0).all()


def _seam_dirs():
    """exact_directions() plus near_seams(rng, 600, N_k) for N_k in (4, 2, 1), seed 0: 74 + 3 * 1200 = 3674 = 11 * 334 slots."""
    rng = np.random.default_rng(0)
    d = np.concatenate([cref.exact_directions()] + [cref.near_seams(rng, 600, Nk) for Nk in (4, 2, 1)])
    return d.reshape(1, 11, 334, 1, 3).astype(np.float32)


def _assert_borders_and_corners(d, Nk):
    st = cref.stage(d, Nk, None, "linear")
    lo_x, hi_x, lo_y, hi_y = st["i0"] == -1, st["i0"] == Nk - 1, st["j0"] == -1, st["j0"] == Nk - 1
    borders = corners = 0
    for f in range(6):
        on = st["face"] == f
        for k, b in enumerate((lo_x, hi_x, lo_y, hi_y)):
            assert (on & b & st["seam"].any(-1)).any(), (Nk, "face", f, "border", k)
            borders += 1
        for bx, by in itertools.product((lo_x, hi_x), (lo_y, hi_y)):
            assert (on & bx & by & (st["miss"] >= 0)).any(), (Nk, "face", f, "a corner")
            corners += 1
    assert (borders, corners) == (24, 24)


@pytest.mark.parametrize("C,per_view", [(3, False), (4, True)])
def test_seams_and_corners_at_every_level_size(C, per_view):
    N = 4
    d = _seam_dirs()
    for Nk in (4, 2, 1):
        _assert_borders_and_corners(d, Nk)
    rng = np.random.default_rng(30 + C)
    tex, mip = _cube(rng, 1, N, C, per_view)
    g = rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32)
    for level in (0.5, 1.5):
        lod = np.full(d.shape[:4], level, np.float32)
        _check_forward(d, lod, tex, mip, None, None, ("seams", level, C))
        _check_grads(d, lod, tex, mip, None, None, g, ("seams", level, C))


# (C, per_view, L, N, max_mip_level, box chain): every value of C, L and N, both sharings, every max_mip_level
GRAD_GRID = [(1, False, 1, 4, None, False), (2, True, 4, 2, None, False), (3, False, 4, 8, None, True), (4, True, 1, 8, 1, False),
             (7, False, 4, 6, None, False), (16, True, 4, 4, None, False), (16, False, 1, 8, None, False), (3, True, 4, 1, None, False),
             (4, False, 4, 5, None, False), (3, False, 1, 8, 0, False)]


def test_gradient_grid_covers_every_axis():
    seen = [set(x) for x in zip(*GRAD_GRID)]
    assert seen == [set(CS), {False, True}, set(LS), set(NS), set(MAX_LEVELS), {False, True}]


@pytest.mark.parametrize("k", range(len(GRAD_GRID)))
def test_gradients_against_float64(k):
    C, per_view, L, N, max_mip_level, box = GRAD_GRID[k]
    d, lod, rl = _inputs(N, L, 200 + k, max_mip_level)
    rng = np.random.default_rng(300 + k)
    tex, mip = _cube(rng, SHAPE[0], N, C, per_view, max_mip_level, box)
    g = rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32)
    _check_forward(d, lod, tex, mip, rl, max_mip_level, GRAD_GRID[k])
    _check_grads(d, lod, tex, mip, rl, max_mip_level, g, GRAD_GRID[k])


def test_sparse_upstream_one_pixel_per_tile():
    """One family of tests/upstream.py: per element |got - float64| <= util.summation_bound(max|float64|, sum |w g|), and
    exactly zero where no term arrives."""
    N, L, C = 8, 4, 3
    d, lod, rl = _inputs(N, L, 400, None, (2, 40, 50))
    tex, mip = _cube(np.random.default_rng(401), 2, N, C, False)
    dense = np.random.default_rng(402).standard_normal(d.shape[:4] + (C,)).astype(np.float32)
    empty = ref.stage(d, lod, N, rl)["empty"]
    g, _ = U.mask_slots("one_pixel_per_tile", dense, (~empty).sum(-1))
    dt, dm, dd, dl = _bwd(d, lod, tex, mip, rl, None, g)
    wt, wm, wd, wl, terms = ref.grads64(d, lod, tex, mip, rl, None, g)
    st, sm, *_ = ref.grads64(d, lod, np.zeros_like(tex), np.zeros_like(mip), rl, None, np.abs(g.astype(np.float64)))
    assert wt.any() and wm.any() and wd.any() and wl.any()
    for name, got, want, sabs in (("tex", dt, wt, st), ("mip", dm, wm, sm)):
        err, bound = np.abs(got - want), summation_bound(float(np.abs(want).max()), sabs)
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
        assert not got[sabs == 0].any(), name
    live = ~empty & (g != 0).any(-1)
    assert not dd[~live].any() and not dl[~live].any()
    assert rel_linf(dd, wd) <= GRAD_TOL and (np.abs(dl - wl) <= _level_bound(wl, terms)).all()


@pytest.mark.parametrize("C", [3, 16])
def test_table_overflow_route(C):
    """Random directions on faces of 64^2 at levels 0 .. 3: every 16 x 16 tile addresses more distinct keys per layer than the
    scatter's LDS table holds; those that find no slot add straight to global memory."""
    N, shape = 64, (2, 32, 32, 2)
    rng = np.random.default_rng(5)
    d = rng.standard_normal(shape + (3,)).astype(np.float32)
    lod = rng.uniform(0.0, 3.0, shape).astype(np.float32)
    least = ref.distinct_keys_per_tile(d, lod, N)
    print("distinct keys per tile and layer, at least", least)
    assert least > table_capacity()
    rl = rng.integers(-1, 6, shape).astype(np.int32)
    for per_view in (False, True):
        tex, mip = _cube(rng, shape[0], N, C, per_view)
        g = rng.standard_normal(shape + (C,), dtype=np.float32)
        _check_forward(d, lod, tex, mip, rl, None, ("overflow", C, per_view))
        _check_grads(d, lod, tex, mip, rl, None, g, ("overflow", C, per_view))


@pytest.mark.parametrize("C", [1, 3, 16])
def test_every_lane_on_the_one_by_one_level(C):
    """Every slot beyond the last level of an N = 4 cube: three-tap corner samples of the six texels of the 1 x 1 level; at 1.5,
    every slot adds to those six and to the 2 x 2 level's 24."""
    N, shape = 4, (2, 50, 70, 4)
    rng = np.random.default_rng(6)
    d = rng.standard_normal(shape + (3,)).astype(np.float32)
    for level, most_keys in ((7.0, 6), (1.5, 30)):
        lod = np.full(shape, level, np.float32)
        assert ref.distinct_keys_per_tile(d, lod, N, worst=max) <= most_keys
        for per_view in (False, True):
            tex, mip = _cube(rng, shape[0], N, C, per_view)
            g = rng.standard_normal(shape + (C,), dtype=np.float32)
            _check_forward(d, lod, tex, mip, None, None, ("hot", level, C, per_view))
            dt, dm, dd, dl = _check_grads(d, lod, tex, mip, None, None, g, ("hot", level, C, per_view))
            assert not dt.any() and (dm[..., :4, :] != 0).any() == (level < 2) and (dm[..., 4, :] != 0).all()


def _renderer():
    mv, proj = scenes.camera(32, 16)
    return dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")


def test_mip_none_builds_the_box_chain():
    """mip=None: tex.grad = the direct gradient + the chain's through texture_mipmaps; texture_mipmaps on a cube per view."""
    N, C, L = 8, 3, 4
    r = _renderer()
    d, lod, rl = _inputs(N, L, 500)
    rng = np.random.default_rng(501)
    g = rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32)
    for per_view in (False, True):
        tex, box = _cube(rng, SHAPE[0], N, C, per_view, None, True)
        chain = r.texture_mipmaps(_cu(tex))
        assert np.array_equal(_bits(_np(chain)), _bits(box)) and chain.shape == tex.shape[:-3] + (ref.layout(N)[2], C)
        t = _cu(tex).requires_grad_(True)
        out = r.texture(_cu(d), t, _cu(rl), "linear-mipmap-linear", "cube", mip_level=_cu(lod))
        assert np.array_equal(_bits(_np(out)), _bits(ref.forward32(d, lod, tex, box, rl)))
        out.backward(_cu(g))
        wt, wm, *_ = ref.grads64(d, lod, tex, box, rl, None, g)
        want = wt + mref.mipmaps_backward64(tex.shape, None, wm)
        assert np.abs(mref.mipmaps_backward64(tex.shape, None, wm)).max() > 0.1 * np.abs(wt).max()
        assert rel_linf(_np(t.grad), want) <= GRAD_TOL
    out1 = r.texture(_cu(d), _cu(tex), _cu(rl), "linear-mipmap-linear", "cube", max_mip_level=1, mip_level=_cu(lod))
    assert np.array_equal(_bits(_np(out1)), _bits(ref.forward32(d, lod, tex, ref.box_chain(tex, 1), rl, 1)))


def test_needs_input_grad():
    N, C, L = 4, 4, 4
    r = _renderer()
    d, lod, rl = _inputs(N, L, 600)
    rng = np.random.default_rng(601)
    tex, mip = _cube(rng, SHAPE[0], N, C, False)
    g = _cu(rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32))
    calls = []
    real = _C.texture_cube_mip_backward_cuda

    def spy(*a):
        calls.append(tuple(a[-4:]))
        return real(*a)
    _C.texture_cube_mip_backward_cuda = spy
    lib = _C.load_library()
    real_b = lib.dm2_texture_cube_mip_backward
    launches = []
    try:
        res = {}
        combos = [(True, True, True, True), (True, False, False, False), (False, True, False, False), (False, False, True, False),
                  (False, False, False, True)]
        for need in combos:
            t, m, u, lv = (_cu(x).requires_grad_(n) for x, n in zip((tex, mip, d, lod), need))
            r.texture(u, t, _cu(rl), "linear-mipmap-linear", "cube", mip=m, mip_level=lv).backward(g)
            res[need] = tuple(None if x.grad is None else x.grad.clone() for x in (t, m, u, lv))
        assert calls == combos                                            # (need_tex, need_mip, need_dirs, need_level)
        for need in combos[1:]:
            k = need.index(True)
            assert [x is not None for x in res[need]] == list(need)
            if k >= 2:                                                    # pure functions of the inputs: the same bits
                assert torch.equal(res[need][k], res[combos[0]][k])
            else:
                assert rel_linf(_np(res[need][k]), _np(res[combos[0]][k])) <= GRAD_TOL
        del calls[:]
        lib.dm2_texture_cube_mip_backward = lambda *a: launches.append(tuple(bool(p.value) for p in a[-4:-1])) or real_b(*a)
        out = r.texture(_cu(d), _cu(tex), _cu(rl), "linear-mipmap-linear", "cube", mip=_cu(mip), mip_level=_cu(lod))
        assert out.grad_fn is None
        w = torch.ones(1, device="cuda", requires_grad=True)
        (out.sum() * w).backward()
        args = (_cu(d), _cu(lod), _cu(tex), _cu(mip), _cu(rl), None, g)
        assert real(*args, False, False, False, False) == (None, None, None, None)
        assert not calls and not launches                                 # nothing asked for: no launch
        real(*args, True, False, False, False)
        real(*args, False, True, False, False)
        real(*args, False, False, False, True)
        assert launches == [(True, False, False), (False, True, False), (False, False, True)]     # the other pointers NULL
    finally:
        _C.texture_cube_mip_backward_cuda = real
        lib.dm2_texture_cube_mip_backward = real_b


@pytest.mark.parametrize("C", [4, 16])
def test_unaligned_views_give_the_same_bits(C):
    """tex, mip and the upstream gradient as views 4 bytes into their storage: the four-channel reads do not apply; the forward
    and the direction / level rows are the same bits as with aligned tensors."""
    N, L = 4, 4
    d, lod, rl = _inputs(N, L, 700)
    rng = np.random.default_rng(701)
    tex, mip = _cube(rng, SHAPE[0], N, C, False)
    g = rng.standard_normal(d.shape[:4] + (C,), dtype=np.float32)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = _cu(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    a = (_cu(d), _cu(lod))
    out_a = _C.texture_cube_mip_cuda(*a, _cu(tex), _cu(mip), _cu(rl))
    out_u = _C.texture_cube_mip_cuda(*a, shifted(tex), shifted(mip), _cu(rl))
    ga = _C.texture_cube_mip_backward_cuda(*a, _cu(tex), _cu(mip), _cu(rl), None, _cu(g), True, True, True, True)
    gu = _C.texture_cube_mip_backward_cuda(*a, shifted(tex), shifted(mip), _cu(rl), None, shifted(g), True, True, True, True)
    assert torch.equal(out_a, out_u) and torch.equal(ga[2], gu[2]) and torch.equal(ga[3], gu[3])
    assert np.array_equal(_bits(_np(out_u)), _bits(ref.forward32(d, lod, tex, mip, rl)))
    wt, wm, *_ = ref.grads64(d, lod, tex, mip, rl, None, g)
    assert rel_linf(_np(gu[0]), wt) <= GRAD_TOL and rel_linf(_np(gu[1]), wm) <= GRAD_TOL


def test_argument_checks():
    d = torch.ones((2, 4, 5, 3, 3), device="cuda")
    lod = torch.ones((2, 4, 5, 3), device="cuda")
    tex = torch.zeros((6, 8, 8, 3), device="cuda")
    mip = torch.zeros((6, 21, 3), device="cuda")
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32, device="cuda")
    ok = _C.texture_cube_mip_cuda(d, lod, tex, mip, rl)
    assert tuple(ok.shape) == (2, 4, 5, 3, 3)
    for args, name in (((d[..., :2], lod, tex, mip, rl), "dirs"), ((d.double(), lod, tex, mip, rl), "dirs"),
                       ((d, lod[..., :2], tex, mip, rl), "mip_level"), ((d, lod.double(), tex, mip, rl), "mip_level"),
                       ((d, lod, tex[:5], mip, rl), "tex"), ((d, lod, tex[:, :7], mip, rl), "tex"), ((d, lod, tex.half(), mip, rl), "tex"),
                       ((d, lod, tex, mip[:, :20], rl), "mip"), ((d, lod, tex, mip[:5], rl), "mip"), ((d, lod, tex, mip.double(), rl), "mip"),
                       ((d, lod, tex, mip[None].expand(2, 6, 21, 3), rl), "mip"), ((d, lod, tex, mip, rl, 1), "mip"),
                       ((d, lod, tex, mip, rl[:1]), "render_layers")):
        with pytest.raises(RuntimeError, match=name):
            _C.texture_cube_mip_cuda(*args)
    assert tuple(_C.texture_cube_mip_cuda(d, lod, tex, mip[:, :16], rl, 1).shape) == (2, 4, 5, 3, 3)
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.texture_cube_mip_backward_cuda(d, lod, tex, mip, rl, None, ok[..., :2], True, True, True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_cube_mip_cuda(d, lod.cpu(), tex, mip, rl)
    with pytest.raises(RuntimeError, match="boundary_mode"):              # the 2D wrapper does not know the mode
        _C.texture_mip_cuda(d[..., :2], torch.zeros((2, 4, 5, 3, 4), device="cuda"), tex[0], mip[0], rl, "cube")
    r = _renderer()
    for kw in (dict(), dict(filter_mode="linear-mipmap-linear"), dict(boundary_mode="clamp"), dict(filter_mode="nearest", boundary_mode="cube"),
               dict(boundary_mode="cube")):
        with pytest.raises(ValueError, match="mip_level"):
            r.texture(d, tex, rl, mip_level=lod, **kw)
    with pytest.raises(ValueError, match="boundary_mode"):
        r.texture(d, tex, rl, "linear-mipmap-linear", "cube", uv_da=torch.zeros((2, 4, 5, 3, 4), device="cuda"), mip_level=lod)
    with pytest.raises(ValueError, match="boundary_mode"):
        r.texture(d, tex, rl, "linear-mipmap-linear", "cube", mip=mip)
    assert torch.equal(r.texture(d, tex, rl, "linear-mipmap-linear", "cube", mip=mip, mip_level=lod), ok)
    # degenerate sizes: zeros without a launch
    lib = _C.load_library()
    real_f, real_b = lib.dm2_texture_cube_mip, lib.dm2_texture_cube_mip_backward
    launches = []
    try:
        lib.dm2_texture_cube_mip = lambda *a: launches.append("f") or real_f(*a)
        lib.dm2_texture_cube_mip_backward = lambda *a: launches.append("b") or real_b(*a)
        for shape in ((0, 4, 5, 2), (2, 0, 5, 2), (2, 4, 5, 0)):
            d0, l0 = torch.ones(shape + (3,), device="cuda"), torch.ones(shape, device="cuda")
            out = _C.texture_cube_mip_cuda(d0, l0, tex, mip, None)
            assert tuple(out.shape) == shape + (3,)
            dt, dm, dd, dl = _C.texture_cube_mip_backward_cuda(d0, l0, tex, mip, None, None, torch.ones_like(out), True, True, True, True)
            assert tuple(dd.shape) == shape + (3,) and tuple(dl.shape) == shape and not dt.any() and not dm.any()
        assert not launches
    finally:
        lib.dm2_texture_cube_mip, lib.dm2_texture_cube_mip_backward = real_f, real_b
    # the C ABI: the cube's chain has its own two symbols; boundary 2, its word under ABI 7, is unknown to the 2D ops
    p = lambda t: _C._ptr(t)
    rows = torch.zeros((2, 4, 5, 3, 4), device="cuda")
    assert lib.dm2_texture_cube_mip(2, 4, 5, 3, 8, 3, 0, -1, p(rl), p(d), p(lod), p(tex), p(mip), p(ok), None) == 0
    assert lib.dm2_texture_cube_mip(2, 4, 5, 3, 18919, 3, 0, 0, p(rl), p(d), p(lod), p(tex), p(mip), p(ok), None) == 1
    assert lib.dm2_texture_cube_mip(2, 4, 5, 3, 8, 3, 0, -1, p(rl), p(d), p(lod), p(tex), None, p(ok), None) == 1
    assert lib.dm2_texture_cube_mip_backward(2, 4, 5, 3, 8, 3, 0, -1, p(rl), p(d), p(lod), p(tex), p(mip), p(ok), None, None, p(rows),
                                             None) == 0
    assert lib.dm2_texture_cube_mip_backward(2, 4, 5, 3, 18919, 3, 0, 0, p(rl), p(d), p(lod), p(tex), p(mip), p(ok), None, None,
                                             p(rows), None) == 1
    assert lib.dm2_texture_cube_mip_backward(2, 4, 5, 3, 8, 3, 0, -1, p(rl), p(d), p(lod), p(tex), p(mip), p(ok), None, None,
                                             ctypes_offset(rows, 4), None) == 1
    for boundary in (2, 7):
        assert lib.dm2_texture_mip(2, 4, 5, 3, 8, 8, 3, 0, boundary, -1, p(rl), p(d), p(lod), p(tex), p(mip), p(ok), None) == 1
        assert lib.dm2_texture_mip_backward(2, 4, 5, 3, 8, 8, 3, 0, boundary, -1, p(rl), p(d), p(lod), p(tex), p(mip), p(ok), None, None,
                                            p(rows), None) == 1
    assert lib.dm2_texture(2, 4, 5, 3, 8, 8, 3, 0, 1, 2, p(rl), p(d), p(tex), p(ok), None) == 1
    assert lib.dm2_texture_backward(2, 4, 5, 3, 8, 8, 3, 0, 1, 2, p(rl), p(d), p(tex), p(ok), None, p(rows), None) == 1
    torch.cuda.synchronize()


def ctypes_offset(t, nbytes):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + nbytes)


def test_module_path_end_to_end():
    """rasterize -> interpolate(vertex_normals) -> shading_vectors -> texture(reflection, cube chain, mip_level = per-face
    roughness x (nlev - 1)) -> composite -> a random-weighted sum, on rasterize_ref's soup scene, against the same chain of
    numpy references: the gradients of the roughness, of the cube and of the vertices."""
    W, H, bidx, L, C, N = 90, 70, [2, 0, 2], 4, 3, 8
    sc = scenes.triangle_soup(W, H, 1000, scenes.SEED_BASE + 80, num_cams=3, depth_complexity=30.0, shared_verts=True).to("cuda")
    s = rref.scene("soup")
    assert np.array_equal(s["verts"], _np(sc.verts)) and np.array_equal(s["faces"], _np(sc.faces))
    r = dm2.LayeredRenderer(sc.mv, sc.proj, W, H, "cuda")
    assert type(r).texture is dm2.Renderer.texture
    faces, F = sc.faces, sc.faces.shape[0]
    nlev = ref.layout(N)[0]
    gen = torch.Generator().manual_seed(17)
    tex0 = torch.randn((6, N, N, C), generator=gen).cuda()
    rough0 = (torch.rand((F,), generator=gen) * 0.9 + 0.05).cuda()
    alpha0 = torch.rand((F,), generator=gen).cuda() * 0.8 + 0.1
    bg = torch.tensor([0.2, -0.1, 0.5]).cuda()
    verts, tex, rough = (x.clone().requires_grad_(True) for x in (sc.verts, tex0, rough0))
    layers, cnt, bary, t = r.rasterize(bidx, verts, faces, L)
    vn = r.vertex_normals(verts, faces)
    nimg = r.interpolate(layers, bary, vn, faces)
    pos, view, nrm, refl = r.shading_vectors(bidx, layers, t, nimg)
    level = rough[layers.clamp(min=0).long()] * (nlev - 1)
    shaded = r.texture(refl, tex, layers, "linear-mipmap-linear", "cube", mip_level=level)
    out, acc = r.composite(shaded, alpha0, layers, bg)
    wgt = torch.randn(out.shape, generator=gen).cuda()
    (out * wgt).sum().backward()
    torch.cuda.synchronize()
    assert int(cnt.sum()) > 3000
    for x in (tex.grad, verts.grad, rough.grad):
        assert x is not None and torch.isfinite(x).all() and x.abs().max() > 0
    # the references, op by op, each at the float32 values the pipeline had
    rl, refln, lvn, texn = _np(layers), _np(refl), _np(level), _np(tex0)
    box = ref.box_chain(texn)
    assert np.array_equal(_bits(_np(shaded)), _bits(ref.forward32(refln, lvn, texn, box, rl)))
    _, _, _, n_contrib = _C.composite_cuda(shaded.detach(), alpha0, layers, bg)
    dvalues, _ = composite_ref.grads64(_np(shaded), _np(alpha0), rl, _np(bg), _np(n_contrib), _np(wgt))
    wt, wm, wd, wl, _ = ref.grads64(refln, lvn, texn, box, rl, None, dvalues)
    want_tex = wt + mref.mipmaps_backward64(texn.shape, None, wm)
    live = rl >= 0
    want_rough = np.bincount(rl[live], weights=wl[live] * (nlev - 1), minlength=F)
    pm = torch.zeros((len(bidx), 2), dtype=torch.int32, device="cuda")
    ro, rd = (_np(x) for x in r.select_rays(bidx, pm, W, H))
    dt, dn, _, _ = shading_ref.grads64(rl, _np(t), _np(nimg), ro, rd, None, None, wd)
    dvn, dbary = interpolate_ref.grads64(rl, _np(bary), _np(vn), _np(faces), dn)
    want_verts = normals_ref.grads64(_np(sc.verts), _np(faces), dvn)[0] + rref.grads64(_np(sc.verts), _np(faces), rl, ro, rd, dbary, dt)
    e_tex, e_rough, e_verts = rel_linf(_np(tex.grad), want_tex), rel_linf(_np(rough.grad), want_rough), rel_linf(_np(verts.grad), want_verts)
    print("module path: tex.grad", e_tex, "roughness.grad", e_rough, "verts.grad", e_verts)
    assert np.abs(want_tex).max() > 0 and np.abs(want_rough).max() > 0 and np.abs(want_verts).max() > 0
    assert e_tex <= GRAD_TOL and e_rough <= GRAD_TOL and e_verts <= GRAD_TOL
