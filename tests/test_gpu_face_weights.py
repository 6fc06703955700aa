"""Per-face blend weights: Renderer.forward(..., return_face_weights=True), LayeredRenderer.render(..., return_face_weights=True),
the ``_C.face_weights_output`` side channel and the C entry points under them (out_face_weights of dm2_forward, dm2_forward_run and
dm2_layers_composite).

face_weights[b, f] is the sum of alpha * T over the blends of face f in view b.  The reference is the colour op's own gradient
through an identity: with every vertex colour (1, 1, 1), dL/dcolor = (1, 0, 0) and dL/ddepth = 0, dL/dfaces_intense[b, f] =
sum (i0 + i1 + i2) alpha T, and the clamped barycentrics sum to 1.  The CPU oracle, the HIP backward and the layered
restatement (tests/layer_composite_ref.py, tests/face_weights_ref.py) serve as references unchanged."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import layer_composite_ref as lref
from face_weights_ref import layered_face_weights64
from util import from_image_oracle_args, rel_linf, scenes, soup_args, to_numpy_args
from util import spy_library as _spy_library

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _orc():
    from oracle import cpu as orc
    return orc


def _dev(args):
    return [a.cuda() if torch.is_tensor(a) else a for a in args]


@contextlib.contextmanager
def _flags(f):
    old = _C.set_flags(f)
    try:
        yield
    finally:
        _C.set_flags(old)


def unit_color(args):
    a = list(args)
    a[6] = torch.ones_like(a[6])
    return a


def oracle_weights(nargs):
    """dL/dfaces_intense of the float32 oracle on the unit-colour scene for dL/dcolor = (1, 0, 0): the face weights."""
    orc = _orc()
    na = list(nargs)
    na[6] = np.ones_like(na[6])
    ref = orc.render_forward_cuda(*na, nthreads=orc.max_threads())
    B, H, W = ref.depth.shape
    gc = np.zeros((B, H, W, 3), np.float32); gc[..., 0] = 1.0
    g = orc.render_backward_cuda(ref, gc, np.zeros((B, H, W), np.float32), nthreads=orc.max_threads())
    return g["faces_intense"], ref


def check_weights(got, want, min_nonzero=10):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    want = np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got > 0, want != 0), (int(((got > 0) != (want != 0)).sum()))
    assert not (got < 0).any()
    assert (got > 0).sum() >= min_nonzero
    assert rel_linf(got, want) <= TOL, rel_linf(got, want)


def _soup(seed, temp=1.0, K=20, B2=True, W=160, H=112, F=700, dc=4.0, batch_idx=(1, 0)):
    if B2:
        return soup_args(W, H, F, scenes.SEED_BASE + seed, temp=temp, K=K, cams=2, batch_idx=batch_idx,
                         patch_min=[[16, 8], [40, 32]], pw=96, ph=64, depth_complexity=dc)[0]
    return soup_args(W, H, F, scenes.SEED_BASE + seed, temp=temp, K=K, depth_complexity=dc)[0]


# ---- 1. oracle parity through the _C op ------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [1.0, 0.0])
@pytest.mark.parametrize("K", [20, 0])
@pytest.mark.parametrize("route", ["default", "no_backward", "no_pair_pool", "legacy"])
def test_weights_match_oracle(temp, K, route):
    """B = 2 patches at offsets of two cameras: face_weights against the oracle's unit-colour dL/dfaces_intense; colour and
    depth bit-equal to the call without weights."""
    args = _soup(91, temp, K)
    want, _ = oracle_weights(to_numpy_args(args))
    dargs = _dev(args)
    flags = {"legacy": _C.DM2_FLAG_LEGACY_KERNELS, "no_pair_pool": _C.DM2_FLAG_NO_PAIR_POOL}.get(route, 0)
    with _flags(flags), _C.forward_only(route == "no_backward"):
        plain = _C.render_forward_cuda(*dargs)
        with _C.face_weights_output(True):
            out = _C.render_forward_cuda(*dargs)
    torch.cuda.synchronize()
    assert len(plain) == 10 and len(out) == 11
    for i in (1, 2, 5):
        assert torch.equal(out[i], plain[i]), i
    assert out[10].shape == (2, dargs[5].shape[0])
    check_weights(out[10], want)


def test_weights_repeated_camera():
    """B = 2 views of the same camera, different patches."""
    args = _soup(92, batch_idx=(0, 0))
    want, _ = oracle_weights(to_numpy_args(args))
    with _C.face_weights_output(True):
        out = _C.render_forward_cuda(*_dev(args))
    check_weights(out[10], want)


def test_weights_with_alpha_after_it():
    """alpha_output and face_weights_output together: alpha at 10, weights at 11; sum_f weights == sum_px alpha."""
    args = _soup(93)
    want, ref = oracle_weights(to_numpy_args(args))
    with _C.face_weights_output(True), _C.alpha_output(True):
        out = _C.render_forward_cuda(*_dev(args))
    assert len(out) == 12
    check_weights(out[11], want)
    a = out[10].double().sum((1, 2)).cpu().numpy()
    s = out[11].double().sum(-1).cpu().numpy()
    assert np.abs(s - a).max() <= TOL * np.abs(a).max()


def test_weights_large_triangles_classes():
    """Triangles of ~130 pixels: the forward's class-by-class route (candidate pairs per list entry >= 32)."""
    args = _soup(94, B2=False, W=128, H=128, F=500)
    want, _ = oracle_weights(to_numpy_args(args))
    with _C.face_weights_output(True):
        out = _C.render_forward_cuda(*_dev(args))
    assert _C.last_pair_bound() >= 32 * out[0]
    check_weights(out[10], want)


def test_weights_tables_from_image():
    """Placeholder AA tables built by the plan from verts_image (the benchmarked route)."""
    from dmesh2_renderer_amd.sharding import BandShardedOp
    args = _soup(95)
    want, _ = oracle_weights(from_image_oracle_args(args))
    a = BandShardedOp(_dev(args), 1, 0, tables_from_image=True).args
    with _C.aa_grad_to_verts(True), _C.tables_from_image(True), _C.face_weights_output(True):
        out = _C.render_forward_cuda(*a)
    check_weights(out[10], want)


def test_weights_over_budget_rerun_not_doubled():
    """The pair pool turns out over budget after the first composite: render_forward_cuda renders again with masks only
    (dm2_forward rendered with a pool, dm2_forward_run renders again); the weights are those of ONE composite."""
    args = _soup(96)
    want, _ = oracle_weights(to_numpy_args(args))
    dargs = _dev(args)
    with _C.face_weights_output(True):
        _C.render_forward_cuda(*dargs)                  # (sizes the binning buffer of this shape for a pool: one C call next)
    lib = _C.load_library()
    modes = []

    def fwd(*a):
        rc = lib.dm2_forward(*a)
        modes.append((rc, a[-1]._obj.value))
        return rc

    runs = []

    def run(*a):
        runs.append(1)
        return lib.dm2_forward_run(*a)

    budget = _C._pool_budget
    _C._pool_budget = lambda N, R: 1
    try:
        with _spy_library(dm2_forward=fwd, dm2_forward_run=run), _C.face_weights_output(True):
            out = _C.render_forward_cuda(*dargs)
    finally:
        _C._pool_budget = budget
    assert modes == [(0, _C.FWD_POOL)] and runs == [1], (modes, runs)
    assert _C.last_forward_mode() == _C.FWD_MASKS
    check_weights(out[10], want)


# ---- 2. identities on the GPU ------------------------------------------------------------------------------------------------
PREPS = [dict(fused_prep=False), dict(fused_prep=True, tables_from_image=False), dict(fused_prep=True, tables_from_image=True),
         dict(fused_prep=True, tables_from_image=True, analytic_rays=True), dict(fused_prep=False, analytic_rays=True)]


def _hip_identity(r, sc, bidx, pm, pw, ph, temp):
    """dL/dfaces_intense of the HIP backward on the unit-colour scene for dL/dcolor = (1, 0, 0), through the module."""
    inten = sc.faces_intense[bidx].clone().requires_grad_(True)
    out = r(bidx, pm, pw, ph, sc.verts, sc.faces, torch.ones_like(sc.verts_color), sc.faces_opacity, inten, sc.background,
            aa_temperature=temp)
    out[0][..., 0].sum().backward()
    torch.cuda.synchronize()
    return inten.grad


@pytest.mark.parametrize("temp", [1.0, 0.0])
@pytest.mark.parametrize("prep", range(len(PREPS)))
def test_module_every_prep(prep, temp):
    """Renderer.forward on every host prep, B = 2 patches at offsets: weights against the HIP backward identity, sum against
    the alpha image, colour / depth / alpha bit-equal to the call without weights, gradients within 1e-5, no grad on the
    weights, and the same weights under torch.no_grad()."""
    W, H = 160, 112
    sc = scenes.triangle_soup(W, H, 700, scenes.SEED_BASE + 97, num_cams=2, shared_verts=True).to("cuda")
    r = dm2.Renderer(sc.mv, sc.proj, W, H, "cuda", **PREPS[prep])
    bidx, pm, pw, ph = [1, 0], torch.tensor([[16, 8], [40, 32]], device="cuda"), 96, 64
    want = _hip_identity(r, sc, bidx, pm, pw, ph, temp)
    g = torch.Generator().manual_seed(21)
    wc, wd = torch.randn((2, ph, pw, 3), generator=g).cuda(), torch.randn((2, ph, pw), generator=g).cuda()
    res = []
    for rw in (False, True):
        leaves = [sc.verts.clone().requires_grad_(True), sc.verts_color.clone().requires_grad_(True),
                  sc.faces_opacity.clone().requires_grad_(True), sc.faces_intense[bidx].clone().requires_grad_(True)]
        out = r(bidx, pm, pw, ph, leaves[0], sc.faces, leaves[1], leaves[2], leaves[3], sc.background, aa_temperature=temp,
                return_alpha=True, return_face_weights=rw)
        ((out[0] * wc).sum() + (out[1] * wd).sum() + out[2].sum()).backward()
        torch.cuda.synchronize()
        res.append((out, [x.grad for x in leaves]))
    (o0, g0), (o1, g1) = res
    assert len(o0) == 3 and len(o1) == 4
    for i in range(3):
        assert torch.equal(o0[i], o1[i]), i
    fw = o1[3]
    assert not fw.requires_grad and fw.grad_fn is None
    check_weights(fw, want.cpu().numpy())
    a = o1[2].detach().double().sum((1, 2))
    assert (fw.double().sum(-1) - a).abs().max().item() <= TOL * a.abs().max().item()
    for a0, a1 in zip(g0, g1):
        assert rel_linf(a1.cpu().numpy(), a0.cpu().numpy()) <= TOL
    with torch.no_grad():
        ng = r(bidx, pm, pw, ph, sc.verts, sc.faces, sc.verts_color, sc.faces_opacity, sc.faces_intense[bidx], sc.background,
               aa_temperature=temp, return_face_weights=True)
    assert len(ng) == 3 and torch.equal(ng[0], o0[0])
    check_weights(ng[2], want.cpu().numpy())


def test_module_color_only_loss():
    """face_weights returned, only colour in the loss: backward works and gives the two-output gradients."""
    W, H = 96, 64
    sc = scenes.triangle_soup(W, H, 500, scenes.SEED_BASE + 98, shared_verts=True).to("cuda")
    r = dm2.Renderer(sc.mv, sc.proj, W, H, "cuda")
    grads = []
    for rw in (False, True):
        v = sc.verts.clone().requires_grad_(True)
        out = r([0], torch.zeros((1, 2), dtype=torch.int64, device="cuda"), W, H, v, sc.faces, sc.verts_color,
                sc.faces_opacity, sc.faces_intense, sc.background, return_face_weights=rw)
        assert len(out) == (3 if rw else 2)
        out[0].sum().backward()
        grads.append(v.grad)
        if rw:
            assert out[2].shape == (1, sc.faces.shape[0]) and not out[2].requires_grad
    assert rel_linf(grads[1].cpu().numpy(), grads[0].cpu().numpy()) <= TOL


def test_cfg2_full_frame_against_hip_backward():
    """bench cfg 2 (512 x 512, 50 k faces): the weights against the HIP backward's unit-colour dL/dfaces_intense."""
    import sys
    from util import ROOT
    sys.path.insert(0, ROOT)
    import bench
    args, _, _, (W, H, F) = bench.build_inputs("cfg2", torch.device("cuda", 0), 0, 1)
    assert (W, H, F) == (512, 512, 50_000)
    uargs = unit_color(args)
    with _C.face_weights_output(True):
        out = _C.render_forward_cuda(*uargs)
    B = out[1].shape[0]
    gc = torch.zeros((B, H, W, 3), device="cuda"); gc[..., 0] = 1.0
    g = _C.render_backward_cuda(out[0], *uargs, gc, torch.zeros((B, H, W), device="cuda"), out[7], out[8], out[9], out[3],
                                out[4], out[5], out[6])
    torch.cuda.synchronize()
    check_weights(out[10], g[4].cpu().numpy(), min_nonzero=1000)


# ---- 3. early-outs and the C ABI -------------------------------------------------------------------------------------------------
def test_early_outs_are_zeros():
    """F == 0, P == 0 and an empty patch (N == 0): the early-out of render_forward_cuda gives zeros of shape (B, F)."""
    args = list(_soup(99, B2=False, W=64, H=48, F=50))
    a0 = list(args)                                             # F == 0
    a0[5] = a0[5][:0]; a0[7] = a0[7][:0]; a0[10] = a0[10][:, :0]
    for k in range(12, 18):
        a0[k] = a0[k][:, :0]
    with _C.face_weights_output(True):
        out = _C.render_forward_cuda(*_dev(a0))
    assert out[0] == 0 and out[10].shape == (1, 0) and out[10].dtype == torch.float32
    a1 = list(a0)                                               # P == 0 (and no faces)
    a1[4] = a1[4][:0]; a1[6] = a1[6][:0]; a1[8] = a1[8][:, :0]; a1[9] = a1[9][:, :0]
    with _C.face_weights_output(True):
        out = _C.render_forward_cuda(*_dev(a1))
    assert out[10].shape == (1, 0)
    a2 = list(args)                                             # N == 0: a 0 x 0 patch
    a2[2] = a2[3] = 0
    a2[19], a2[20] = a2[19][:, :0, :0], a2[20][:, :0, :0]
    with _C.face_weights_output(True), _C.alpha_output(True):
        out = _C.render_forward_cuda(*_dev(a2))
    assert len(out) == 12 and out[11].shape == (1, 50) and out[11].dtype == torch.float32 and not out[11].any()


def _null(p):
    """Is this ctypes argument a NULL pointer (None, or a c_void_p of 0)?"""
    return p is None or getattr(p, "value", p) in (None, 0)


def test_null_weights_pointer_is_the_old_call():
    """A caller that asks for nothing extra gets the plain path: with no side channel set, every optional slot of the C calls
    (weights, alpha gradient, window) is NULL, on the one-call and on the plan-then-run route; dm2_layers_composite with NULL
    window and NULL weights is composite_layers_cuda, bit for bit; and asking for the weights does not perturb the image."""
    args = _dev(_soup(100))
    sc = lref.ortho_scene(B=2, H=21, W=19, L=4, F=7, seed=3)
    la = _layer_args(sc)
    lib = _C.load_library()
    calls = {"dm2_forward": 0, "dm2_forward_run": 0, "dm2_backward": 0, "dm2_layers_composite": 0, "dm2_layers_composite_backward": 0}
    optional = {"dm2_forward": (10,), "dm2_forward_run": (13,), "dm2_backward": (5,), "dm2_layers_composite": (1, 6),
                "dm2_layers_composite_backward": (1, 4)}

    def spy(name):
        def f(*a):
            calls[name] += 1
            assert all(_null(a[i]) for i in optional[name]), (name, [a[i] for i in optional[name]])
            return getattr(lib, name)(*a)
        return f

    plain = _C.render_forward_cuda(*args)
    with _spy_library(**{name: spy(name) for name in calls}):
        _C._bin_hint.clear()                                     # (no binning buffer at hand: the plan-then-run route too)
        nulled = _C.render_forward_cuda(*args)
        gc, gd = torch.ones_like(nulled[1]), torch.ones_like(nulled[2])
        _C.render_backward_cuda(nulled[0], *args, gc, gd, nulled[7], nulled[8], nulled[9], *nulled[3:7])
        shim = _C.composite_layers_cuda(*la)
        _C.composite_layers_backward_cuda(*la, shim[3], torch.ones_like(shim[0]), torch.ones_like(shim[1]))
    assert calls == {"dm2_forward": 1, "dm2_forward_run": 1, "dm2_backward": 1, "dm2_layers_composite": 1,
                     "dm2_layers_composite_backward": 1}, calls
    for i in (1, 2, 5):
        assert torch.equal(plain[i], nulled[i]), i
    with _C.face_weights_output(True):
        weighted = _C.render_forward_cuda(*args)
    for i in (1, 2, 5):                                          # (the WEIGHTS kernels only add work beside the blend)
        assert torch.equal(plain[i], weighted[i]), i
    # the layered entry point, called directly
    keep = []
    d, dev = _C._composite_desc(*la, keep)
    direct = [torch.empty_like(x) for x in shim]
    assert lib.dm2_layers_composite(ctypes.byref(d), None, *[_C._ptr(x) for x in direct], None, _C._stream(dev)) == 0
    torch.cuda.synchronize()
    for x, y in zip(shim, direct):
        assert torch.equal(x, y)


# ---- 4. the layered path ----------------------------------------------------------------------------------------------------------
def _layer_args(inp):
    t = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).cuda() for k, v in inp.items()}
    return [t[k] for k in ("render_layers", "verts", "faces", "verts_color", "faces_opacity", "faces_intense", "verts_ndc",
                           "background", "ray_o", "ray_d")]


def _check_layered(inp, min_nonzero):
    args = _layer_args(inp)
    F = args[2].shape[0]
    plain = _C.composite_layers_cuda(*args)
    with _C.face_weights_output(True):
        out = _C.composite_layers_cuda(*args)
    assert len(plain) == 4 and len(out) == 5
    for x, y in zip(plain, out[:4]):
        assert torch.equal(x, y)
    fwd = lref.forward32(*[a.cpu() for a in args])
    want = layered_face_weights64(fwd, args[4].cpu().numpy(), F)
    check_weights(out[4], want, min_nonzero)
    # the unit-colour identity through LayeredCompositeFunction's intense gradient
    uargs = list(args)
    uargs[3] = torch.ones_like(args[3])
    inten = args[5].clone().requires_grad_(True)
    uargs[5] = inten
    with _C.face_weights_output(True):
        color, depth, fw = dm2.LayeredCompositeFunction.apply(*uargs)
    assert not fw.requires_grad
    color[..., 0].sum().backward()
    torch.cuda.synchronize()
    check_weights(fw, inten.grad.cpu().numpy(), min_nonzero)
    return fwd


@pytest.mark.parametrize("L", [5, 10, 12])
def test_layered_hand_built_lists(L):
    """Holes, out-of-range ids, a face repeated in a pixel's list (counted twice), opacities of exactly 0 and 1.  L = 5, 10,
    12: ids read one at a time, as pairs and as vectors of four (k_layer_composite<1 / 2 / 4, true>)."""
    sc = lref.ortho_scene(B=2, H=37, W=45, L=L, F=11, seed=L + 50)
    rl = sc["render_layers"]
    rl[:, ::3, :, 1] = rl[:, ::3, :, 0]
    sc["faces_opacity"][[2, 5]] = [0.0, 1.0]
    fwd = _check_layered(sc, min_nonzero=3)
    assert fwd["blend"].sum() > 100


@pytest.mark.parametrize("name", list(lref.CROWDED))
def test_layered_table_overflow_route(name):
    """k_layer_composite<4, true> where the face table overflows or is nearly full (test_gpu_layer_composite.py's crowded
    scenes): the blends that find no slot add alpha * T straight to face_weights[b, f]; B = 2, so the b * F offset counts."""
    from test_gpu_layer_composite import crowded
    sc = crowded(name, "face weights")
    fwd = _check_layered(sc, min_nonzero=int(0.8 * sc["faces"].shape[0]))
    want = layered_face_weights64(fwd, sc["faces_opacity"], sc["faces"].shape[0])
    assert (want[0] > 0).sum() > 0.5 * want.shape[1] and (want[1] > 0).sum() > 0.5 * want.shape[1]
    assert rel_linf(want[0], want[1]) > 0.1                                   # (the views' rows differ)


def test_layered_cfg3_and_module():
    """cfg 3 (1024^2, tet_lattice(n=25), L = 4 from generate) and LayeredRenderer.render(return_face_weights=True)."""
    W = H = 1024
    ts = scenes.tet_lattice(W, H, 25, seed=scenes.SEED_BASE + 3).to("cuda")
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda")
    layers, _ = lr.generate([0], ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, 4)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    ndc, _ = lr.compute_verts_ndc_image(ts.verts, ts.mv[[0]], ts.proj[[0]])
    rng = np.random.RandomState(22)
    inp = dict(render_layers=layers, verts=ts.verts, faces=ts.faces, verts_ndc=ndc.contiguous(),
               ray_o=lr.ray_o[[0]].contiguous(), ray_d=lr.ray_d[[0]].contiguous(),
               verts_color=rng.uniform(0, 1, (P, 3)).astype(np.float32), faces_opacity=rng.uniform(0.05, 0.95, F).astype(np.float32),
               faces_intense=rng.uniform(0.5, 1.5, (1, F)).astype(np.float32), background=np.array([0.1, 0.3, 0.7], np.float32))
    _check_layered(inp, min_nonzero=1000)
    vc, op, it = (torch.from_numpy(inp[k]).cuda() for k in ("verts_color", "faces_opacity", "faces_intense"))
    bg = torch.from_numpy(inp["background"]).cuda()
    o0 = lr.render([0], layers, ts.verts, ts.faces, vc, op, it, bg, return_alpha=True)
    o1 = lr.render([0], layers, ts.verts, ts.faces, vc, op, it, bg, return_alpha=True, return_face_weights=True)
    assert len(o1) == 4 and all(torch.equal(a, b) for a, b in zip(o0, o1[:3]))
    a = o1[2].double().sum()
    assert abs(o1[3].double().sum() - a).item() <= TOL * a.item()
    with torch.no_grad():
        o2 = lr.render([0], layers, ts.verts, ts.faces, vc, op, it, bg, return_face_weights=True)
    assert len(o2) == 3 and rel_linf(o2[2].cpu().numpy(), o1[3].cpu().numpy()) <= TOL


def test_layered_empty():
    sc = lref.ortho_scene(B=2, H=9, W=8, L=3, F=5, seed=4)
    sc["render_layers"][:] = -1
    with _C.face_weights_output(True):
        out = _C.composite_layers_cuda(*_layer_args(sc))
    assert out[4].shape == (2, 5) and not out[4].any()
