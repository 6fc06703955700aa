"""Every backward under sparse upstream gradients (tests/upstream.py): the Renderer op on each of its backward routes, and the
deferred layer ops, against their float64 references.

Renderer: one forward per (scene, route), one backward per family on that forward, the dense gradient last (the sparse runs
left no state behind).  Per element  |g_hip - g64| <= GRAD_TOL max|g64| + 8 eps32 sum|per-pixel terms|  (util.summation_bound),
exactly zero where no pixel of the support contributes.  The AA tensor is held to the same bound on every route: no element of
the polygon-free Jacobian (pool) or the segment clipper (masks only) needed the clippers' own per-pair tolerance on top of it.
Each run prints a line per tensor: the worst element, its bound, its sum of |terms|."""
import contextlib

import numpy as np
import pytest
import torch

import upstream as U
from test_gpu_tie_queue import witness
from util import GRAD_NAMES, GRAD_TOL, check_backward, from_image_oracle_args, rel_linf, to_dev

from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

ROUTES = ("pool", "masks_only", "point", "legacy", "from_image", "alpha")
HALVES = (U.IMAGE_FAMILIES[:6], U.IMAGE_FAMILIES[6:])
QUEUED = ("pool", "from_image", "alpha")          # the routes whose backward runs the tie pass


def _context(scene, route, family):
    ctx = U.context(scene, route == "point", family)
    if route == "from_image":                     # the tables the plan builds from verts_image are the scene's own
        na = from_image_oracle_args(ctx.args)
        for k in range(12, 18):
            assert np.array_equal(np.asarray(na[k]), np.asarray(ctx.na[k]), equal_nan=True), k
    return ctx


@contextlib.contextmanager
def _route(route, backward=False):
    flags = _C.DM2_FLAG_LEGACY_KERNELS if route == "legacy" else 0
    old, budget = _C.set_flags(flags), _C._pool_budget
    try:
        with contextlib.ExitStack() as st:
            if route == "masks_only" and not backward:
                _C._pool_budget = lambda N, R: 0
            if route == "from_image":
                st.enter_context(_C.tables_from_image(True)); st.enter_context(_C.aa_grad_to_verts(True))
            if route == "alpha" and not backward:
                st.enter_context(_C.alpha_output(True))
            yield
    finally:
        _C._pool_budget = budget
        _C.set_flags(old)


def _forward(ctx, route):
    dargs = to_dev(ctx.args)
    if route == "from_image":
        from dmesh2_renderer_amd.sharding import BandShardedOp
        dargs = BandShardedOp(dargs, 1, 0, tables_from_image=True).args
        assert dargs[12].shape[1] == 0
    with _route(route):
        out = _C.render_forward_cuda(*dargs)
    want = {"legacy": _C.FWD_NONE, "point": _C.FWD_POINT, "masks_only": _C.FWD_MASKS}.get(route, _C.FWD_POOL)
    assert _C.last_forward_mode() == want, (route, _C.last_forward_mode())
    assert np.array_equal(out[1].cpu().numpy().view(np.uint32), ctx.r32.color.view(np.uint32))
    return dargs, out


def _backward(route, dargs, out, gc, gd, gA):
    kw = {} if gA is None else dict(dL_dout_alpha=torch.from_numpy(gA).cuda())
    with _route(route, backward=True):
        g = _C.render_backward_cuda(out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(), out[7], out[8], out[9],
                                    out[3], out[4], out[5], out[6], **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in g]


def _aa_form(route, ctx, x):
    return U.routed(x, ctx.na) if route == "from_image" else x


@pytest.mark.parametrize("half", [0, 1], ids=["families_a", "families_b"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("scene", U.SCENES)
def test_renderer_sparse_upstream(scene, route, half):
    alpha = route == "alpha"
    forwards = {}                                                                 # one forward per window the families are seen through
    worst = {}
    for family in HALVES[half]:
        ctx = _context(scene, route, family)
        if ctx.window not in forwards:
            forwards[ctx.window] = (ctx,) + _forward(ctx, route)
        _, dargs, out = forwards[ctx.window]
        ref = ctx.reference(family, alpha)
        g = _backward(route, dargs, out, ref["gc"], ref["gd"], ref["gA"])
        assert not g[3][..., :2].any()                                            # verts_ndc: only z receives gradient
        for name, x in zip(GRAD_NAMES, g):
            aa = name == "aa_face_verts"
            form = (lambda v: _aa_form(route, ctx, v)) if aa else (lambda v: v)
            held = None if ref["held32"] is None else ref["held32"][name]
            if held is not None and aa and route == "from_image":
                held = form(held.astype(np.float64)) > 0
            line, ratio, which = U.check_tensor(name, x, form(ref["g64"][name]), form(ref["sabs"][name]), g32=form(ref["g32"][name]),
                                                held32=held, what=f"{scene} {route} {family}")
            print(line)
            if ratio > worst.get(name, (0.0,))[0]:
                worst[name] = (ratio, which, family)
        if family == "all_zero":
            assert all(not x.any() for x in g), [n for n, x in zip(GRAD_NAMES, g) if x.any()]
        if route in QUEUED and family in ("depth_only", "all_zero"):
            n, direct = witness(out)                                              # the queue as this backward's tie pass saw it
            if family == "all_zero":
                assert n == 0 and direct == 0, (n, direct)                        # nothing queued, nothing by the direct route
            elif scene == "lattice":
                assert n > 0, n                                                   # (the words are live: the run before all_zero queued)
    print(f"WORST {scene} {route} " + ", ".join(f"{k} {v[0]:.3g} ({v[1]}, {v[2]})" for k, v in worst.items()))
    # the dense gradient again, as check_backward accepts it: the sparse runs left no state behind
    for ctx, dargs, out in forwards.values():
        g = _backward(route, dargs, out, ctx.gc, ctx.gd, ctx.gA if alpha else None)
        gref = _dense_reference(ctx, alpha)
        if scene == "lattice" and route in QUEUED:
            n, direct = witness(out)
            assert n > 64 and direct == 0, (n, direct)                            # the lattice still drains mid-tile and never fills
        if route == "from_image":
            want = U.routed(gref["aa_face_verts"], ctx.na)
            assert g[5].shape == want.shape
            assert rel_linf(g[5], want) <= GRAD_TOL, rel_linf(g[5], want)
            g[5] = gref["aa_face_verts"]
        check_backward(dict(grads=g, ref_grads=gref))


_DENSE = {}


def _dense_reference(ctx, alpha):
    """The fp32 oracle's gradients under the dense upstream gradient (with ``alpha``: plus the zero-channel scene's)."""
    from oracle import cpu as orc
    key = (ctx.scene, ctx.point, ctx.window, alpha)
    if key not in _DENSE:
        g = orc.render_backward_cuda(ctx.r32, ctx.gc, ctx.gd, nthreads=ctx.nt)
        if alpha:
            z32, _ = ctx._zero_channel()
            cz = np.zeros_like(ctx.gc); cz[..., 2] = ctx.gA
            a = orc.render_backward_cuda(z32, cz, np.zeros_like(ctx.gd), nthreads=ctx.nt)
            for n in GRAD_NAMES:
                if n != "verts_color":
                    g[n] = (g[n].astype(np.float64) + a[n]).astype(np.float32)
        _DENSE[key] = g
    return _DENSE[key]


# ---- material axes (upstream.material_args): factors a one-camera soup multiplies by 1 or 0 ------------------------------------
_MATERIAL = {}
MATERIAL_CASES = [(s, t, r) for s, t in U.MATERIAL_SCENES for r in (("point",) if t == 0.0 else tuple(x for x in ROUTES if x != "point"))]


class _Material:
    """A scene under upstream.material_args with both oracles' forwards and the float64 gradients under the scene's dense
    upstream gradient, with and without the alpha image's; computed once and shared by the routes."""

    def __init__(self, scene, temp):
        from oracle import cpu as orc
        from util import to_numpy_args
        self.args = U.material_args(scene, temp)
        self.na = to_numpy_args(self.args)
        self.nt = min(orc.max_threads(), 16)
        self.r32 = orc.render_forward_cuda(*self.na, nthreads=self.nt)
        r64 = orc.render_forward_cuda(*self.na, dtype=np.float64, nthreads=self.nt)
        assert np.array_equal(self.r32.n_contrib, r64.n_contrib)                   # (the two oracles take the same branches here)
        B, H, W = self.r32.depth.shape
        self.gc, self.gd, self.gA = U.dense_upstream(scene, B, H, W, alpha=True)
        self.g64 = orc.render_backward_cuda(r64, self.gc.astype(np.float64), self.gd.astype(np.float64), nthreads=self.nt)
        z64 = orc.render_forward_cuda(*U.zero_channel_np(self.na), dtype=np.float64, nthreads=self.nt)
        cz = np.zeros(self.gc.shape); cz[..., 2] = self.gA
        a64 = orc.render_backward_cuda(z64, cz, np.zeros(self.gd.shape), nthreads=self.nt)
        self.g64_alpha = {n: self.g64[n] + (0.0 if n == "verts_color" else a64[n]) for n in GRAD_NAMES}


@pytest.mark.parametrize("scene,temp,route", MATERIAL_CASES, ids=[f"{s}-{'own' if t is None else t}-{r}" for s, t, r in MATERIAL_CASES])
def test_material_axes(scene, temp, route):
    """A background with a negative and a > 1 component, signed colours, intensities per (view, face) with exact zeros and exact
    0 and 1 opacities on the ragged 50 x 37 (temperature 0.5, and 0: the point route) and the two-view patch, on every backward
    route: the forward bit for bit against the fp32 oracle, the six gradients at GRAD_TOL against the float64 oracle.
    tests/test_upstream_cpu.py counts what these scenes reach: pixels that end on an alpha-1 contributor, blended faces of
    intensity 0.  Found by the mutation audit: with intensity 1 and a grey or zero background, a swapped
    background channel on the alpha route, a dropped intensity factor and the opaque last contributor's depth term went unseen."""
    from util import check_forward, pool_state
    key = (scene, temp)
    if key not in _MATERIAL:
        _MATERIAL[key] = _Material(scene, temp)
    m = _MATERIAL[key]
    dargs = to_dev(m.args)
    if route == "from_image":
        from dmesh2_renderer_amd.sharding import BandShardedOp
        na = from_image_oracle_args(m.args)
        for k in range(12, 18):
            assert np.array_equal(np.asarray(na[k]), np.asarray(m.na[k]), equal_nan=True), k
        dargs = BandShardedOp(dargs, 1, 0, tables_from_image=True).args
    with _route(route):
        out = _C.render_forward_cuda(*dargs)
    want = {"legacy": _C.FWD_NONE, "point": _C.FWD_POINT, "masks_only": _C.FWD_MASKS}.get(route, _C.FWD_POOL)
    assert _C.last_forward_mode() == want, (route, _C.last_forward_mode())
    check_forward(dict(out=out[:10], ref=m.r32, pool=pool_state(out[:10])), m.args)
    alpha = route == "alpha"
    g = _backward(route, dargs, out, m.gc, m.gd, m.gA if alpha else None)
    gref = dict(m.g64_alpha if alpha else m.g64)
    if route == "from_image":
        want_aa = U.routed(gref["aa_face_verts"], m.na)
        assert g[5].shape == want_aa.shape
        assert rel_linf(g[5], want_aa) <= GRAD_TOL, rel_linf(g[5], want_aa)
        g[5] = gref["aa_face_verts"]
    worst = check_backward(dict(grads=g, ref_grads=gref))
    print(f"materials {scene} {temp} {route}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


_VANISHING = {}


@pytest.mark.parametrize("route", [r for r in ROUTES if r != "point"])
def test_vanishing_temperature(route):
    """aa_temperature = 2^-149 on the ragged 50 x 37: where the ray misses the face, coverage * temperature is 2^-149 for a pair
    that covers more than half its pixel and rounds to exactly 0 for the others, and a pair of zero coverage does not blend
    (forward.cu:379): a quarter of the pixels end on another face than under any usable temperature (counted in
    tests/test_upstream_cpu.py), which only n_contrib and the masks show -- such a pair's alpha is 0.  Forward and integer state
    bit for bit; gradients at GRAD_TOL against the fp32 oracle (the float64 oracle does not round those products to 0: it
    blends other pairs and is no reference here) WITHOUT a record buffer: a pair of zero mixed coverage behind a pixel's last
    contributor has a record the reference's backward never pops, the record-stack desync corner (SURVEY.md appendix A,
    tests/desync_scene.py), where this library's gradients are those of len_oarea_buffer = 0 by design.  Found by the
    mutation audit."""
    from oracle import cpu as orc
    from util import check_forward, pool_state, to_numpy_args
    if not _VANISHING:
        args = U.scene_args("ragged", U.VANISHING_TEMPERATURE)
        na = to_numpy_args(args)
        r32 = orc.render_forward_cuda(*na)
        B, H, W = r32.depth.shape
        gc, gd, gA = U.dense_upstream("ragged", B, H, W, alpha=True)
        n0 = list(na); n0[18] = 0
        r0 = orc.render_forward_cuda(*n0)
        assert np.array_equal(r0.color, r32.color) and np.array_equal(r0.n_contrib, r32.n_contrib)
        g = orc.render_backward_cuda(r0, gc, gd)
        cz = np.zeros_like(gc); cz[..., 2] = gA
        a = orc.render_backward_cuda(orc.render_forward_cuda(*U.zero_channel_np(n0)), cz, np.zeros_like(gd))
        ga = {n: (g[n] if n == "verts_color" else (g[n].astype(np.float64) + a[n]).astype(np.float32)) for n in GRAD_NAMES}
        _VANISHING.update(args=args, na=na, r32=r32, gc=gc, gd=gd, gA=gA, g=g, ga=ga)
    v = _VANISHING
    assert 0.0 < v["na"][11] < 1e-44
    dargs = to_dev(v["args"])
    if route == "from_image":
        from dmesh2_renderer_amd.sharding import BandShardedOp
        dargs = BandShardedOp(dargs, 1, 0, tables_from_image=True).args
    with _route(route):
        out = _C.render_forward_cuda(*dargs)
    want = {"legacy": _C.FWD_NONE, "masks_only": _C.FWD_MASKS}.get(route, _C.FWD_POOL)
    assert _C.last_forward_mode() == want, (route, _C.last_forward_mode())
    check_forward(dict(out=out[:10], ref=v["r32"], pool=pool_state(out[:10])), v["args"])
    alpha = route == "alpha"
    g = _backward(route, dargs, out, v["gc"], v["gd"], v["gA"] if alpha else None)
    gref = dict(v["ga"] if alpha else v["g"])
    if route == "from_image":
        want_aa = U.routed(gref["aa_face_verts"], v["na"])
        assert g[5].shape == want_aa.shape and rel_linf(g[5], want_aa) <= GRAD_TOL
        g[5] = gref["aa_face_verts"]
    print(f"vanishing temperature {route}:", check_backward(dict(grads=g, ref_grads=gref)))


# ---- the deferred ops: each module's own float64 reference and tolerance, under the slot families -------------------------------
def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dense(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _report(what, family, name, got, want):
    e = rel_linf(got, want)
    print(f"{what} {family} {name}: rel L_inf {e:.3g} of max|g64| {float(np.abs(want).max()) if want.size else 0.0:.3g}")
    return e


RASTERIZE = [("lattice", 4), ("lattice", 17), ("overflow_L4", 4)]


@pytest.mark.parametrize("name,L", RASTERIZE, ids=[f"{n}-L{L}" for n, L in RASTERIZE])
def test_rasterize_sparse_upstream(name, L):
    """k_rasterize_bwd skips a slot whose four upstream values are zero: L = 4 (one vector of ids) and 17 (the second pass) on the
    ragged lattice, and the crowded lists whose faces overflow the block's table (the direct atomics, most lanes skipped)."""
    import rasterize_ref as rref
    import test_gpu_rasterize as tr
    if name.startswith("overflow"):
        import layer_composite_ref as lref
        sc, kind = lref.crowded_case(name)
        rl = sc["render_layers"]
        assert kind == "overflow" and rl.shape[-1] == L
        verts, faces, ro, rd = sc["verts"], sc["faces"], sc["ray_o"], sc["ray_d"]
        layers = _cu(rl)
    else:
        s = tr._scene(name)
        layers = _C.rasterize_layers_cuda(*tr._dev(s, s["fe"]), L)[0]
        rl = layers.cpu().numpy()
        verts, faces, ro, rd = s["verts"], s["faces"], s["ray_o"], s["ray_d"]
    B, H, W, _ = rl.shape
    assert H % 16 or W % 16 or name.startswith("overflow")
    F, P = faces.shape[0], verts.shape[0]
    listed = (rl >= 0) & (rl < F)
    weight = listed.sum(-1)
    gb, gt = _dense(rl.shape + (3,), 31 + L), _dense(rl.shape, 32 + L)
    dv, df, dro, drd = _cu(verts), _cu(faces), _cu(ro), _cu(rd)
    for family in U.SLOT_FAMILIES:
        mb, _ = U.mask_slots(family, gb, weight)
        mt = np.zeros_like(gt) if family == "one_channel" else U.mask_slots(family, gt, weight)[0]
        got = _C.rasterize_layers_backward_cuda(layers, dv, df, dro, drd, _cu(mb), _cu(mt)).cpu().numpy()
        torch.cuda.synchronize()
        assert np.isfinite(got).all()
        if family == "all_zero":
            assert not got.any(), family
            continue
        want = rref.grads64(verts, faces, rl, ro, rd, mb, mt)
        if not want.any():                                                        # (the lattice lists fewer than 17 hits: its last layer is empty)
            assert family == "last_layer_only" and L == 17 and not got.any(), family
            continue
        e = _report(f"rasterize {name} L={L}", family, "verts", got, want)
        assert e <= GRAD_TOL, (name, L, family, e)
        live = listed & ((mb != 0).any(-1) | (mt != 0))
        touched = np.zeros(P, dtype=bool)
        touched[faces[rl[live]].reshape(-1)] = True
        assert not got[~touched].any(), (name, L, family)                          # no non-zero upstream slot: exactly 0
        assert (~touched).any()


@pytest.mark.parametrize("label", ["lattice-L3", "overflow"])
def test_coverage_sparse_upstream(label):
    """k_coverage_bwd skips a slot whose upstream value is zero: the ragged lattice at the module's odd L, and its table-overflow
    case."""
    import coverage_ref as cref
    import test_gpu_coverage_op as tcov
    c = cref.scene_case("lattice", 3) if label == "lattice-L3" else cref.overflow_case()
    rl = c["render_layers"]
    weight = (rl >= 0).sum(-1)
    for t in (1.0, 0.5):
        for family in U.slot_families(c["g"]):
            g, _ = U.mask_slots(family, c["g"], weight)
            got = tcov._backward(c, t, g)
            assert np.isfinite(got).all()
            if family == "all_zero":
                assert not got.any(), (label, t)
                continue
            want = cref.grad_image64(rl, c["verts_image"], c["faces"], t, g, c["info"][t])
            assert want.any(), (label, t, family)
            assert not got[want == 0].any(), (label, t, family)                    # exactly zero where the reference is zero
            e = _report(f"coverage {label} t={t}", family, "verts_image", got, want)
            assert e <= GRAD_TOL, (label, t, family, e)


def _interpolate_case(name, L):
    import interpolate_ref as iref
    import test_gpu_interpolate as ti
    if name == "overflow":                                                        # (test_gpu_interpolate.py test_table_overflow_route)
        F, N, shape = 5000, 3000, (2, 48, 64, 4)
        rl = np.random.RandomState(5).randint(0, F, shape).astype(np.int32)
        from util import table_capacity
        assert iref.distinct_per_tile(rl) > table_capacity()
        rng = np.random.RandomState(6)
        bary = rng.uniform(0, 1, shape + (3,)).astype(np.float32)
        af = rng.randint(0, N, (F, 3)).astype(np.int32)
        return rl, bary, af, N
    s, rl, bary = ti._rasterized(name, L)
    return rl, bary, s["faces"], s["verts"].shape[0]


INTERPOLATE = [("lattice", 1), ("lattice", 4), ("overflow", 4)]


@pytest.mark.parametrize("name,L", INTERPOLATE, ids=[f"{n}-L{L}" for n, L in INTERPOLATE])
def test_interpolate_sparse_upstream(name, L):
    import interpolate_ref as iref
    import test_gpu_interpolate as ti
    rl, bary, af, N = _interpolate_case(name, L)
    B = rl.shape[0]
    C = 3
    attr = ti._attr(np.random.RandomState(300 + L), B, N, C, True)
    dense = _dense(rl.shape + (C,), 33 + L)
    filled, _ = iref.filled(rl, af, N)
    weight = filled.sum(-1)
    for family in U.slot_families(dense):
        g, _ = U.mask_slots(family, dense, weight)
        da, db = ti._bwd(rl, bary, attr, af, g)
        assert np.isfinite(da).all() and np.isfinite(db).all()
        if family == "all_zero":
            assert not da.any() and not db.any()
            continue
        wa, wb = iref.grads64(rl, bary, attr, af, g)
        assert np.abs(wa).max() > 0 and np.abs(wb).max() > 0, family
        ea, eb = _report(f"interpolate {name} L={L}", family, "attr", da, wa), _report(f"interpolate {name} L={L}", family, "bary", db, wb)
        assert ea <= GRAD_TOL and eb <= GRAD_TOL, (name, L, family, ea, eb)
        live = filled & (g != 0).any(-1)
        assert not db[~live].any(), (name, L, family)                              # no non-zero upstream value: exactly 0
        touched = np.zeros((B, N), dtype=bool)
        b = np.nonzero(live)[0]
        touched[np.repeat(b, 3), af[rl[live]].reshape(-1)] = True
        assert not da[~touched].any() and (~touched).any(), (name, L, family)


TEXTURE = [("lattice", 1, (64, 64)), ("lattice", 4, (5, 3)), ("overflow", 4, (2048, 2048))]


@pytest.mark.parametrize("name,L,size", TEXTURE, ids=[f"{n}-L{L}" for n, L, _ in TEXTURE])
def test_texture_sparse_upstream(name, L, size):
    import test_gpu_texture as tt
    import texture_ref as tref
    C = 3
    if name == "overflow":                                                        # (test_gpu_texture.py test_table_overflow_route)
        from util import table_capacity
        shape = (2, 48, 64, L)
        rng = np.random.default_rng(5)
        uv = rng.uniform(0.0, 1.0, shape + (2,)).astype(np.float32)
        assert tref.distinct_texels_per_tile(uv, *size, None, "linear", "wrap") > table_capacity()
        rl = rng.integers(-1, 6, shape).astype(np.int32)
    else:
        rl, uv = tt._uvs(name, L)
    B = uv.shape[0]
    tex = tt._tex(np.random.default_rng(400 + L), B, size, C, name != "overflow")
    dense = _dense(uv.shape[:4] + (C,), 34 + L)
    empty = tref.empty(uv, size[0], size[1], rl)
    weight = (~empty).sum(-1)
    for family in U.slot_families(dense):
        g, _ = U.mask_slots(family, dense, weight)
        dt, du = tt._bwd(uv, tex, rl, "linear", "wrap", g)
        assert np.isfinite(dt).all() and np.isfinite(du).all()
        if family == "all_zero":
            assert not dt.any() and not du.any()
            continue
        wt, wu = tref.grads64(uv, tex, rl, "linear", "wrap", g)
        assert np.abs(wt).max() > 0 and np.abs(wu).max() > 0, family
        et, eu = _report(f"texture {name} L={L}", family, "tex", dt, wt), _report(f"texture {name} L={L}", family, "uv", du, wu)
        assert et <= GRAD_TOL and eu <= GRAD_TOL, (name, L, family, et, eu)
        live = ~empty & (g != 0).any(-1)
        assert not du[~live].any(), (name, L, family)                              # no non-zero upstream value: exactly 0
        assert not dt[wt == 0].any(), (name, L, family)                            # a texel no live slot samples


IMAGE_OP_FAMILIES = ("one_tile", "one_pixel_per_tile", "lane0", "lane255", "one_colour_channel", "all_zero")


@pytest.mark.parametrize("name", ["hand_built_L5", "overflow"])
def test_layer_composite_sparse_upstream(name):
    """The layer compositor's backward drops zero components before the table or the atomic; its upstream gradients are images,
    so the pixel families and the one-channel family apply: hand-built lists at the module's odd L, and the crowded scene."""
    import layer_composite_ref as lref
    import test_gpu_layer_composite as tl
    if name == "overflow":
        crowd = [k for k in lref.CROWDED if lref.crowded_case(k)[1] == "overflow"][0]
        sc = tl.crowded(crowd, "sparse upstream")
    else:
        sc = lref.ortho_scene(B=2, H=37, W=45, L=5, F=11, seed=5)
        sc["render_layers"][:, ::3, :, 1] = sc["render_layers"][:, ::3, :, 0]
    t = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).cuda() for k, v in sc.items()}
    args = [t[k] for k in ("render_layers", "verts", "faces", "verts_color", "faces_opacity", "faces_intense", "verts_ndc",
                           "background", "ray_o", "ray_d")]
    color, depth, final_T, n_contrib = _C.composite_layers_cuda(*args)
    cpu = [a.cpu() for a in args]
    fwd = lref.forward32(*cpu)
    assert np.array_equal(color.cpu().numpy().view(np.uint32), fwd["color"].view(np.uint32))
    gc, gd = _dense(tuple(color.shape), 35), _dense(tuple(depth.shape), 36)
    weight = fwd["blend"].sum(-1)
    B, F = gd.shape[0], cpu[2].shape[0]
    for family in IMAGE_OP_FAMILIES:
        mc, md, _, mask, _ = U.mask_image(family, gc, gd, None, weight)
        grads = [x.cpu().numpy() for x in _C.composite_layers_backward_cuda(*args, n_contrib, _cu(mc), _cu(md))]
        torch.cuda.synchronize()
        assert all(np.isfinite(x).all() for x in grads)
        if family == "all_zero":
            assert all(not x.any() for x in grads)
            continue
        want = lref.grads64(fwd, cpu[2], cpu[3], cpu[4], cpu[5], cpu[6], cpu[7], torch.from_numpy(mc).double(), torch.from_numpy(md).double())
        for gname, got in zip(tl.GRADS, grads):
            if family == "one_colour_channel" and gname == "verts_ndc":
                assert not got.any() and not np.asarray(want[gname]).any()
                continue
            e = _report(f"layer_composite {name}", family, gname, got, want[gname])
            assert e <= GRAD_TOL, (name, family, gname, e)
        live = fwd["blend"] & ((mc != 0).any(-1) | (md != 0))[..., None]
        touched = np.zeros((B, F), dtype=bool)
        touched[np.nonzero(live)[0], fwd["fs"][live]] = True
        assert not grads[3][~touched].any(), (name, family)                        # faces_intense of a face no live pixel blends
        assert not grads[1][~touched.any(0)].any(), (name, family)                 # faces_opacity


@pytest.mark.parametrize("name", ["L5_C3", "overflow_L4"])
def test_composite_sparse_upstream(name):
    """Renderer.composite's backward: grad_out (B,H,W,C) and grad_acc (B,H,W) under the pixel families and one channel, then
    grad_out sparse with grad_acc dense and the reverse.  Per-face alpha (the scatter through the face table)."""
    import composite_ref as cref
    import test_gpu_composite as tc
    c = dict(cref.case(5, 3, True, True, True) if name == "L5_C3" else cref.crowded(name))
    dense_g, dense_gA = c["g"], c["gA"]
    B, H, W, L, C = c["values"].shape
    assert c["alpha"].ndim == 1
    weight = c["blend"].sum(-1)
    runs = [(f, f) for f in ("one_tile", "one_pixel_per_tile", "lane0", "lane255", "one_channel", "all_zero")]
    runs += [("one_pixel_per_tile", "dense"), ("dense", "one_pixel_per_tile")]

    def cut(family, x):
        if family == "dense":
            return x, np.ones((B, H, W), dtype=bool)
        if family == "all_zero":
            return U.mask_slots("all_zero", x[..., None] if x.ndim == 3 else x)[0].reshape(x.shape), np.zeros((B, H, W), dtype=bool)
        m = U.support(family, B, H, W, weight)
        out = np.where(m.reshape(m.shape + (1,) * (x.ndim - 3)), x, np.zeros_like(x))
        if family == "one_channel":
            if x.ndim == 3:
                return np.zeros_like(x), np.zeros((B, H, W), dtype=bool)
            out[..., :U.ONE_CHANNEL] = 0.0; out[..., U.ONE_CHANNEL + 1:] = 0.0
        return out, m

    for fg, fA in runs:
        (g, mg), (gA, mA) = cut(fg, dense_g), cut(fA, dense_gA)
        c["g"], c["gA"] = np.ascontiguousarray(g), np.ascontiguousarray(gA)
        dv, da = tc._raw_backward(c)
        if fg == "all_zero":
            assert not dv.any() and not da.any()
            continue
        wv, wa = cref.grads64(c["values"], c["alpha"], c["render_layers"], c["background"], c["n_contrib"], c["g"], c["gA"])
        assert np.abs(wa).max() > 0 and np.abs(wv).max() > 0, (fg, fA)
        ev, ea = _report(f"composite {name}", f"{fg}/{fA}", "values", dv, wv), _report(f"composite {name}", f"{fg}/{fA}", "alpha", da, wa)
        tc._close(dv, wv, (name, fg, fA, "dvalues")); tc._close(da, wa, (name, fg, fA, "dalpha"))
        assert not dv[~c["blend"]].any()
        assert not dv[~(mg | mA)].any(), (name, fg, fA)                            # a pixel with no upstream value: exactly 0
        live = c["blend"] & (mg | mA)[..., None]
        touched = np.zeros(c["alpha"].shape[0], dtype=bool)
        touched[c["render_layers"][live]] = True
        assert not da[~touched].any(), (name, fg, fA)
