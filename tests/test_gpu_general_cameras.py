"""The fused prep, the analytic rays and the op under general cameras (tests/cameras.py: three-axis rotations, off-axis
sheared pinholes with non-square pixels), on the GPU against the oracle and float64.

Under ``scenes.camera`` most of the 4x4 arithmetic of csrc/dm2_prep.hip and of analytic_ray (csrc/dm2_device_math.h)
multiplies by exact zeros or by a symmetric block (tests/test_cameras_cpu.py shows that a reassociated sum or a transposed
rotation changes no bit there); here every term counts.

a  prep forward        all eight tensors bit-equal to the oracle
b  prep backward       d(verts) within 1e-6 of the oracle and 1e-5 of float64 autograd, per route; the clamp passes nothing into w
c  camera gradients    test_gpu_camera_grad.check_prep: 1e-5 of the float64 yardstick's largest entry
d  analytic rays       Renderer(analytic_rays=True) against the oracle fed the closed-form rays: images bit-equal, gradients within
                       GRAD_TOL; generate and rasterize bit-equal to the ray-tensor path
e  the op              materialised tables and the tables-from-image path against the oracle
f  module path         verts.grad, mv.grad, proj.grad of Renderer.forward and LayeredRenderer.render against float64 chains
"""
import numpy as np
import pytest
import torch

import cameras
import camera_grad_ref as cgr
import layer_composite_ref as lcr
from test_gpu_camera_grad import check_prep
from util import (GRAD_TOL, capture_forward_args, check_backward, check_forward, check_from_image,
                  from_image_oracle_args, patched_C, pool_state, run_both, scenes, to_numpy_args)

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C
from oracle import cpu as orc

pytestmark = pytest.mark.gpu

W, H, F = 96, 72, 600
SEED = scenes.SEED_BASE + 5
KEYS = ("verts_ndc", "verts_image", "verts", "edges", "iszero", "recip", "normal", "normal_c")
ROUTES = {"ndc": (0,), "image": (1,), "aa": (2,), "all": (0, 1, 2)}
_CACHE = {}


def scene(name):
    """The scenes, built once: soup / grazing (B = 3; P = 1800, eight past a multiple of 256), dense (the dense mix, B = 2),
    large (P = 60003: 235 blocks a view, camera_blocks > 1, B = 3), lattice."""
    if name not in _CACHE:
        _CACHE[name] = {
            "soup": lambda: cameras.reposed_soup(W, H, F, SEED, 3, shared_verts=True),
            "grazing": lambda: cameras.grazing_soup(W, H, F, SEED, 2, shared_verts=True),
            "dense": lambda: cameras.reposed_soup(W, H, F, SEED + 10, 2, mix=cameras.MIX_DENSE, shared_verts=True),
            "large": lambda: cameras.reposed_soup(W, H, 20001, SEED + 20, 3, mix=cameras.MIX_DENSE),
            "lattice": lambda: cameras.reposed_lattice(88, 60, 5, scenes.SEED_BASE + 6, 2),
        }[name]()
        assert name == "lattice" or _CACHE[name].verts.shape[0] % 256 != 0
    return _CACHE[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def legacy_flags(kernels):
    return _C.DM2_FLAG_LEGACY_KERNELS if kernels == "legacy" else 0


def closed_form_rays(ray_cam, width, height):
    cam = ray_cam.cpu().numpy()
    return orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), width, height)


# ---- a. prep forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "grazing", "dense", "large"])
def test_prepare_bit_exact_vs_oracle(name):
    sc = scene(name)
    ref = orc.prepare_faces(sc.verts, sc.faces, sc.mv, sc.proj, W, H)
    outs = _C.prepare_faces(sc.verts.cuda(), sc.faces.cuda(), sc.mv.cuda(), sc.proj.cuda(), W, H)
    torch.cuda.synchronize()
    got = dict(zip(KEYS, [o.cpu().numpy() for o in outs]))
    for k in KEYS:
        assert np.array_equal(bits(got[k]), bits(ref[k])), (k, int((bits(got[k]) != bits(ref[k])).sum()))
    flipped = np.any(got["verts"][:, :, 1] != got["verts_image"][:, sc.faces.numpy()[:, 1]], axis=-1)
    assert flipped.any(axis=1).all() and (~flipped).any(axis=1).all()          # both windings in every view
    if name == "grazing":
        pos, neg = cgr.clamp_masks(sc.verts, sc.mv, sc.proj)
        assert pos[-1].sum() >= 8 and neg[-1].sum() >= 8 and np.abs(got["verts_image"]).max() > 1e5


# ---- b. prep backward, d(verts) ----------------------------------------------------------------------------------------
def upstreams(sc, seed):
    B, P, Fc = sc.mv.shape[0], sc.verts.shape[0], sc.faces.shape[0]
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(s, generator=g) for s in ((B, P, 3), (B, P, 2), (B, Fc, 3, 2)))


@pytest.fixture(scope="module")
def prep_refs():
    """Per scene: upstream gradients, the oracle's tables, and per route the oracle's fp32 and the float64 d(verts)."""
    out = {}
    for name in ("soup", "grazing"):
        sc = scene(name)
        gs = upstreams(sc, 21)
        tabs = orc.prepare_faces(sc.verts, sc.faces, sc.mv, sc.proj, W, H)
        per = {}
        for route, use in ROUTES.items():
            kw = {("g_ndc", "g_image", "g_aa")[i]: gs[i] for i in use}
            o32 = orc.prepare_faces_backward(sc.verts, sc.faces, sc.mv, sc.proj, W, H, **kw)
            f64 = cgr.camera_grads(sc.verts, sc.mv, sc.proj, W, H, faces=sc.faces, aa_face_verts=tabs["verts"],
                                   verts_image=tabs["verts_image"], **kw)["verts"]
            per[route] = (o32, f64)
        out[name] = (gs, per)
    return out


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["soup", "grazing"])
def test_prepare_backward_vs_oracle_and_float64(name, route, prep_refs):
    sc = scene(name).to("cuda")
    gs, per = prep_refs[name]
    o32, f64 = per[route]
    kw = {("g_verts_ndc", "g_verts_image", "g_aa_face_verts")[i]: gs[i].cuda() for i in ROUTES[route]}
    got = _C.prepare_faces_backward(sc.verts, sc.faces.to(torch.int32), sc.mv, sc.proj, W, H, **kw).cpu().numpy()
    print(f"{name} {route}: d(verts) against the oracle {rel(got, o32):.3g}, against float64 {rel(got, f64):.3g}")
    assert np.abs(f64).max() > 0
    assert rel(got, o32) <= 1e-6
    assert rel(got, f64) <= 1e-5


@pytest.mark.parametrize("route", list(ROUTES))
def test_clamped_vertices_pass_no_gradient_into_w(route):
    """The grazing view alone: every row of d(verts) within 1e-5 of the float64 chain whose clamped w is a constant, and so
    the rows of the clamped vertices by themselves (a gradient through w would be 1 / |w| = 1e4 times theirs)."""
    sc = scene("grazing")
    pos, neg = cgr.clamp_masks(sc.verts, sc.mv, sc.proj)
    cl = (pos | neg)[-1].numpy()
    assert cl.sum() >= 20
    gs = [g[-1:] for g in upstreams(sc, 22)]
    mv, proj = sc.mv[-1:], sc.proj[-1:]
    tabs = orc.prepare_faces(sc.verts, sc.faces, mv, proj, W, H)
    use = ROUTES[route]
    f64 = cgr.camera_grads(sc.verts, mv, proj, W, H, faces=sc.faces, aa_face_verts=tabs["verts"], verts_image=tabs["verts_image"],
                           **{("g_ndc", "g_image", "g_aa")[i]: gs[i] for i in use})["verts"]
    kw = {("g_verts_ndc", "g_verts_image", "g_aa_face_verts")[i]: gs[i].cuda() for i in use}
    got = _C.prepare_faces_backward(sc.verts.cuda(), sc.faces.cuda().to(torch.int32), mv.cuda(), proj.cuda(), W, H, **kw).cpu().numpy()
    print(f"grazing view alone, {route}: all rows {rel(got, f64):.3g}, clamped rows {rel(got[cl], f64[cl]):.3g}")
    assert rel(got, f64) <= 1e-5 and rel(got[cl], f64[cl]) <= 1e-5


# ---- c. camera gradients -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "grazing"])
def test_prep_camera_grads_vs_yardstick(name):
    sc = scene(name).to("cuda")
    g_ndc, g_img, g_aa = (g.cuda() for g in upstreams(sc, 23))
    # (welded vertices: the aa route's scatter is not bit-reproducible)
    check_prep(sc.verts, sc.faces.to(torch.int32), sc.mv, sc.proj, W, H, g_ndc, g_img, g_aa, False)


# ---- d. analytic rays --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [1.0, 0.0])
@pytest.mark.parametrize("kernels", ["dense", "legacy"])
def test_renderer_analytic_rays_vs_oracle(temp, kernels):
    """Renderer(analytic_rays=True) and the op under its side channel against the oracle's own render of the op's arguments,
    the ray tensors replaced by the oracle's closed form of the module's ray_cam, cut to each patch."""
    sc = scene("soup").to("cuda")
    bidx, pw, ph = [2, 0], 60, 41
    pm = torch.tensor([[16, 8], [5, 3]], dtype=torch.int64, device="cuda")
    seen = {}
    real = _C.render_forward_cuda

    def spy(*args):
        seen["args"] = args
        return real(*args)

    old = _C.set_flags(legacy_flags(kernels))
    try:
        ra = dm2.Renderer(sc.mv, sc.proj, W, H, "cuda", analytic_rays=True, tables_from_image=False)
        assert ra.ray_o is None and ra.ray_d is None
        with patched_C(render_forward_cuda=spy), torch.no_grad():
            color, depth = ra(bidx, pm, pw, ph, sc.verts, sc.faces, sc.verts_color, sc.faces_opacity, sc.faces_intense[bidx],
                              sc.background, aa_temperature=temp)
        dargs = [a.detach() if torch.is_tensor(a) else a for a in seen["args"]]
        assert dargs[19].numel() == 0 and dargs[12].shape[1] == F
        ro, rd = closed_form_rays(ra.ray_cam, W, H)
        pmn = pm.cpu().numpy()
        cut = lambda r: np.stack([r[c, y:y + ph, x:x + pw] for c, (x, y) in zip(bidx, pmn)])      # noqa: E731
        ref_args = to_numpy_args(dargs)
        ref_args[19], ref_args[20] = cut(ro), cut(rd)
        ref = orc.render_forward_cuda(*ref_args, nthreads=orc.max_threads())
        rng = np.random.RandomState(8)
        gc = rng.randn(*ref.color.shape).astype(np.float32); gd = rng.randn(*ref.depth.shape).astype(np.float32)
        with _C.analytic_rays(ra.ray_cam[bidx].contiguous(), W, H):
            out = _C.render_forward_cuda(*dargs)
            pool = pool_state(out)
            grads = _C.render_backward_cuda(out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(),
                                            out[7], out[8], out[9], out[3], out[4], out[5], out[6])
        res = dict(out=out, pool=pool, ref=ref, grads=[g.cpu().numpy() for g in grads],
                   ref_grads=orc.render_backward_cuda(ref, gc, gd, nthreads=orc.max_threads()))
    finally:
        _C.set_flags(old)
    check_forward(res, ref_args)                                      # colour, depth, tri_cnt (and the plan) bit-equal
    print(f"analytic rays t{temp} {kernels}:", check_backward(res))   # the six gradients within GRAD_TOL
    assert ref.num_rendered > 0 and (ref.final_T < 1).mean() > 0.5
    # the module's own images are those bits too
    assert np.array_equal(bits(color.cpu().numpy()), bits(ref.color))
    assert np.array_equal(bits(depth.cpu().numpy()), bits((1.0 - (ref.depth + np.float32(1.0)) / np.float32(2.0)).astype(np.float32)))


def test_generate_and_rasterize_analytic_rays():
    """LayeredRenderer(analytic_rays=True).generate and Renderer.rasterize: layers, counts, bary and t bit-equal to the
    ray-tensor path fed the same closed-form rays."""
    ts = scene("lattice").to("cuda")
    Wl, Hl, bidx = ts.width, ts.height, [1, 0]
    la = dm2.LayeredRenderer(ts.mv, ts.proj, Wl, Hl, "cuda", analytic_rays=True)
    ro, rd = closed_form_rays(la.ray_cam, Wl, Hl)
    lt = dm2.LayeredRenderer(ts.mv, ts.proj, Wl, Hl, "cuda")
    lt.ray_o, lt.ray_d = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    gen = [r.generate(bidx, ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, 4) for r in (la, lt)]
    assert torch.equal(gen[0][0], gen[1][0]) and torch.equal(gen[0][1], gen[1][1])
    assert ((gen[0][1] > 0).float().mean(dim=(1, 2)) >= 0.5).all()
    ras = [r.rasterize(bidx, ts.verts, ts.faces, 6, faces_existence=ts.faces_existence) for r in (la, lt)]
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(ras[0], ras[1])):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), ("layers", "cnt", "bary", "t")[k]
    assert (ras[0][1] > 0).sum() > 1000
    # and both equal the oracle's walk on the projection and rays they got
    ndc, img = (x.cpu() for x in _C.prepare_faces(ts.verts, ts.faces, ts.mv[bidx], ts.proj[bidx], Wl, Hl)[:2])
    rl, rc = orc.generate_render_layers_cuda(Wl, Hl, ts.verts.cpu(), ts.faces.cpu(), ts.tets.cpu(), ts.face_tets.cpu(), ts.tet_faces.cpu(),
                                             ts.faces_existence.cpu(), ndc, img, ro[bidx], rd[bidx], 4, nthreads=orc.max_threads())
    assert np.array_equal(gen[0][0].cpu().numpy(), rl) and np.array_equal(gen[0][1].cpu().numpy(), rc)


# ---- e. the op ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("kernels", ["dense", "legacy"])
def test_op_vs_oracle(temp, kernels):
    """The fused prep's arguments (capture_forward_args on the GPU) through the op with materialised tables, then through the
    tables-from-image path bench.py runs; three patches at different offsets of views 2, 0, 1."""
    sc = scene("soup")
    pw, ph = 64, 48
    args, _ = capture_forward_args(sc, [2, 0, 1], [[16, 8], [0, 0], [32, 24]], pw, ph, temp=temp, device="cuda")
    args = [a.detach() if torch.is_tensor(a) else a for a in args]
    old = _C.set_flags(legacy_flags(kernels))
    try:
        res = run_both(args, seed=int(10 * temp), nthreads=orc.max_threads())
        check_forward(res, args)
        print(f"op t{temp} {kernels}:", check_backward(res))
        assert res["ref"].num_rendered > 0 and (res["ref"].final_T < 1).mean() > 0.5
        g = torch.Generator().manual_seed(11)
        wc, wd = torch.randn((3, ph, pw, 3), generator=g).cuda(), torch.randn((3, ph, pw), generator=g).cuda()
        print(f"op t{temp} {kernels} from image:", check_from_image(args, wc, wd, tol=GRAD_TOL, nthreads=orc.max_threads()))
    finally:
        _C.set_flags(old)


# ---- f. module path ----------------------------------------------------------------------------------------------------
def per_camera(ref, idx, n):
    out = np.zeros((n, 4, 4))
    for i, b in enumerate(idx):
        out[b] += ref[i]
    return out


def test_renderer_module_gradients_vs_float64_chain():
    """Renderer.forward (default fused prep: tables from image, AA gradient routed to the vertices) + loss.backward().

    Reference: the oracle's op gradients (of verts, verts_ndc and aa_face_verts) for the very arguments the op got, pushed
    through float64 autograd of the prep (camera_grad_ref) to verts, mv and proj.  Bar: max(1e-5, 4 x the reference-alone
    figure) of the largest entry, the reference-alone figure being the same op gradients pushed through the oracle's own fp32
    prepare_faces_backward, against that float64 chain (the 4 allows for the order of the atomic sums).

    Measured on MI355X: reference alone 9.0e-8 (bar 1e-5); HIP verts.grad 2.2e-7, mv.grad 3.0e-7, proj.grad 2.0e-7."""
    sc = scene("soup").to("cuda")
    idx, pw, ph = [2, 0], 80, 60
    pm = torch.tensor([[8, 4], [16, 12]], dtype=torch.int64, device="cuda")
    mv, proj = sc.mv.clone().requires_grad_(True), sc.proj.clone().requires_grad_(True)
    verts = sc.verts.clone().requires_grad_(True)
    r = dm2.Renderer(mv, proj, W, H, "cuda")
    seen = {}
    real = _C.render_forward_cuda

    def spy(*args):
        seen["args"] = args
        return real(*args)

    with patched_C(render_forward_cuda=spy):
        color, depth = r(idx, pm, pw, ph, verts, sc.faces, sc.verts_color, sc.faces_opacity, sc.faces_intense[idx], sc.background)
    g = torch.Generator().manual_seed(31)
    wc, wd = torch.randn(color.shape, generator=g), torch.randn(depth.shape, generator=g)
    ((color * wc.cuda()).sum() + (depth * wd.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert seen["args"][12].shape[1] == 0                              # the default path: placeholders for the tables
    na = from_image_oracle_args(seen["args"])
    ref = orc.render_forward_cuda(*na, nthreads=orc.max_threads())
    assert np.array_equal(bits(color.detach().cpu().numpy()), bits(ref.color))
    gop = orc.render_backward_cuda(ref, wc.numpy(), (wd * -0.5).numpy(), nthreads=orc.max_threads())     # depth = 1 - (z + 1) / 2
    mvb, prb = sc.mv[idx].cpu(), sc.proj[idx].cpu()
    chain = cgr.camera_grads(sc.verts.cpu(), mvb, prb, W, H, g_ndc=gop["verts_ndc"], g_aa=gop["aa_face_verts"], faces=na[5],
                             aa_face_verts=na[12], verts_image=na[9])
    want_v = gop["verts"].astype(np.float64) + chain["verts"]
    alone = gop["verts"].astype(np.float64) + orc.prepare_faces_backward(sc.verts.cpu(), na[5], mvb, prb, W, H, g_ndc=gop["verts_ndc"],
                                                                         g_aa=gop["aa_face_verts"])
    fig = rel(alone, want_v)
    bar = max(1e-5, 4 * fig)
    ev = rel(verts.grad.cpu().numpy(), want_v)
    em = rel(mv.grad.cpu().numpy(), per_camera(chain["mv"], idx, 3))
    ep = rel(proj.grad.cpu().numpy(), per_camera(chain["proj"], idx, 3))
    print(f"Renderer module path: reference alone {fig:.3g} (bar {bar:.3g}); HIP verts.grad {ev:.3g}, mv.grad {em:.3g}, proj.grad {ep:.3g}")
    assert np.abs(chain["mv"]).max() > 0 and np.abs(chain["proj"]).max() > 0 and not mv.grad[1].any()
    assert ev <= bar and em <= bar and ep <= bar


def test_layered_render_module_gradients_vs_float64_chain():
    """LayeredRenderer.render on generate's layers, fused prep, analytic rays, cameras that require grad.

    Reference: layer_composite_ref on the oracle's fp32 projection and closed-form rays (forward bit-equal), its float64
    gradient of verts_ndc pushed through float64 autograd of the prep to verts, mv and proj; bar and reference-alone figure
    as in test_renderer_module_gradients_vs_float64_chain.

    Measured on MI355X: reference alone 1.2e-7 (bar 1e-5); HIP verts.grad 1.8e-7, mv.grad 6.4e-8, proj.grad 6.1e-8."""
    ts = scene("lattice").to("cuda")
    Wl, Hl, bidx = ts.width, ts.height, [1, 0]
    P, Fl = ts.verts.shape[0], ts.faces.shape[0]
    gen = torch.Generator().manual_seed(8)
    color_p = torch.rand((P, 3), generator=gen)
    opac = 0.2 + 0.7 * torch.rand((Fl,), generator=gen)
    intense = 0.75 + 0.5 * torch.rand((2, Fl), generator=gen)
    bg = torch.tensor([0.1, 0.2, 0.3])
    wc, wd = torch.randn((2, Hl, Wl, 3), generator=gen), torch.randn((2, Hl, Wl), generator=gen)
    mv, proj = ts.mv.clone().requires_grad_(True), ts.proj.clone().requires_grad_(True)
    lr = dm2.LayeredRenderer(mv, proj, Wl, Hl, "cuda", fused_prep=True, analytic_rays=True)
    with torch.no_grad():
        layers, _ = lr.generate(bidx, ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, 4)
    verts = ts.verts.clone().requires_grad_(True)
    color, depth = lr.render(bidx, layers, verts, ts.faces, color_p.cuda(), opac.cuda(), intense.cuda(), bg.cuda())
    ((color * wc.cuda()).sum() + (depth * wd.cuda()).sum()).backward()
    torch.cuda.synchronize()
    mvb, prb = ts.mv[bidx].cpu(), ts.proj[bidx].cpu()
    ndc = orc.prepare_faces(ts.verts.cpu(), ts.faces.cpu(), mvb, prb, Wl, Hl)["verts_ndc"]
    ro, rd = closed_form_rays(lr.ray_cam, Wl, Hl)
    fwd = lcr.forward32(layers.cpu(), ts.verts.cpu(), ts.faces.cpu(), color_p, opac, intense, ndc, bg, ro[bidx], rd[bidx])
    assert fwd["blend"].sum() > 1000
    assert np.array_equal(bits(color.detach().cpu().numpy()), bits(fwd["color"]))
    want = lcr.grads64(fwd, ts.faces.cpu(), color_p, opac, intense, ndc, bg, wc.double(), (wd * -0.5).double())
    chain = cgr.camera_grads(ts.verts.cpu(), mvb, prb, Wl, Hl, g_ndc=want["verts_ndc"])
    alone = orc.prepare_faces_backward(ts.verts.cpu(), ts.faces.cpu(), mvb, prb, Wl, Hl, g_ndc=want["verts_ndc"].astype(np.float32))
    fig = rel(alone, chain["verts"])
    bar = max(1e-5, 4 * fig)
    ev = rel(verts.grad.cpu().numpy(), chain["verts"])
    em = rel(mv.grad.cpu().numpy(), per_camera(chain["mv"], bidx, 2))
    ep = rel(proj.grad.cpu().numpy(), per_camera(chain["proj"], bidx, 2))
    print(f"LayeredRenderer.render: reference alone {fig:.3g} (bar {bar:.3g}); HIP verts.grad {ev:.3g}, mv.grad {em:.3g}, proj.grad {ep:.3g}")
    assert np.abs(chain["mv"]).max() > 0 and np.abs(chain["verts"]).max() > 0
    assert ev <= bar and em <= bar and ep <= bar
