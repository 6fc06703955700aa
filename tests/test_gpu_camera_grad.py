"""Camera-matrix gradients of the fused host prep (dm2_prepare_faces_backward_camera) on the GPU.

Prep level: ``_C.prepare_faces_backward(..., need_camera=True)`` within 1e-5 of the largest entry of the float64 yardstick
(camera_grad_ref.py) for each upstream route and all together, on the shapes of test_gpu_prep.py and on degenerate and
clamped inputs; its d(verts) bit-equal to the verts-only call's; two calls bit-equal; empty inputs give zeros.
Module level: Renderer / LayeredRenderer.render hand mv.grad / proj.grad to cameras that require grad on every fused prep
variant, within the module bar (1e-3 relative, see test_gpu_prep.test_renderer_fused_prep_end_to_end) of the
reference-shaped torch prep, and within 1e-5 of the yardstick fed with the upstream gradients the op actually sent."""
import numpy as np
import pytest
import torch

import camera_grad_ref as cgr
from util import scenes

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C, prep

pytestmark = pytest.mark.gpu

CASES = [
    dict(W=64, H=48, F=300, seed=41, cams=1),
    dict(W=100, H=70, F=1000, seed=42, cams=3),
    dict(W=128, H=128, F=5000, seed=43, cams=2, shared=True),
    dict(W=1920, H=1080, F=20000, seed=44, cams=3),
]
ROUTES = ("ndc", "image", "aa", "all")
BAR = 1e-5


def mixed_orientation(sc):
    f = sc.faces.clone()
    f[1::2] = f[1::2][:, [0, 2, 1]]
    sc.faces = f
    return sc


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def upstream(route, g_ndc, g_img, g_aa):
    return dict(g_verts_ndc=g_ndc if route in ("ndc", "all") else None, g_verts_image=g_img if route in ("image", "all") else None,
                g_aa_face_verts=g_aa if route in ("aa", "all") else None)


def check_prep(verts, faces, mv, proj, W, H, g_ndc, g_img, g_aa, deterministic_scatter):
    """All four routes: camera gradients against the yardstick, d(verts) against the verts-only call, two calls."""
    tabs = _C.prepare_faces(verts, faces, mv, proj, W, H)
    for route in ROUTES:
        kw = upstream(route, g_ndc, g_img, g_aa)
        gv, gm, gp = _C.prepare_faces_backward(verts, faces, mv, proj, W, H, need_camera=True, **kw)
        gv2, gm2, gp2 = _C.prepare_faces_backward(verts, faces, mv, proj, W, H, need_camera=True, **kw)
        old = _C.prepare_faces_backward(verts, faces, mv, proj, W, H, **kw)
        ref = cgr.camera_grads(verts, mv, proj, W, H, g_ndc=kw["g_verts_ndc"], g_image=kw["g_verts_image"],
                               g_aa=kw["g_aa_face_verts"], faces=faces, aa_face_verts=tabs[2], verts_image=tabs[1])
        assert np.abs(ref["mv"]).max() > 0, route
        assert cgr.rel_to_max(gm.cpu().numpy(), ref["mv"]) <= BAR, (route, cgr.rel_to_max(gm.cpu().numpy(), ref["mv"]))
        assert cgr.rel_to_max(gp.cpu().numpy(), ref["proj"]) <= BAR, (route, cgr.rel_to_max(gp.cpu().numpy(), ref["proj"]))
        if kw["g_aa_face_verts"] is None or deterministic_scatter:
            # (a vertex shared by faces takes its aa_face_verts corners by float atomics, in no fixed order)
            assert np.array_equal(bits(gv), bits(old)), route
            assert np.array_equal(bits(gv2), bits(gv)) and np.array_equal(bits(gm2), bits(gm)) and np.array_equal(bits(gp2), bits(gp))
        else:
            assert rel(gv.cpu(), old.cpu()) <= 1e-6 and rel(gm2.cpu(), gm.cpu()) <= 1e-6 and rel(gp2.cpu(), gp.cpu()) <= 1e-6
        # verts-only callers see no change; camera-only refinement writes no d(verts)
        gn, gm3, gp3 = _C.prepare_faces_backward(verts, faces, mv, proj, W, H, need_verts=False, need_camera=True, **kw)
        assert gn is None
        if kw["g_aa_face_verts"] is None or deterministic_scatter:
            assert np.array_equal(bits(gm3), bits(gm)) and np.array_equal(bits(gp3), bits(gp))


@pytest.mark.parametrize("c", CASES)
def test_prep_camera_grads_vs_yardstick(c):
    W, H = c["W"], c["H"]
    sc = mixed_orientation(scenes.triangle_soup(W, H, c["F"], scenes.SEED_BASE + c["seed"], num_cams=c["cams"],
                                                shared_verts=c.get("shared", False))).to("cuda")
    B, P, F = c["cams"], sc.verts.shape[0], sc.faces.shape[0]
    gen = torch.Generator().manual_seed(c["seed"])
    g_ndc, g_img, g_aa = (torch.randn(s, generator=gen).cuda() for s in ((B, P, 3), (B, P, 2), (B, F, 3, 2)))
    check_prep(sc.verts, sc.faces.to(torch.int32), sc.mv, sc.proj, W, H, g_ndc, g_img, g_aa, not c.get("shared", False))


def test_prep_camera_grads_degenerate_and_clamped():
    """test_gpu_prep's degenerate inputs (zero-area faces, repeated vertices, axis-parallel edges, |w| < 1e-4 of both signs
    and w = 0) under two views, the second a rotated and shifted camera."""
    verts = torch.tensor([[0.0, 0.0, 0.5], [0.3, 0.0, 0.5], [0.3, 0.2, 0.5], [0.0, 0.2, 0.5],
                          [0.1, 0.1, 0.00005], [0.2, -0.1, -0.00005], [0.5, 0.5, 0.0], [0.4, 0.4, 2.0]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 3], [0, 2, 1], [0, 0, 1], [4, 5, 6], [1, 1, 1], [7, 4, 2]], dtype=torch.int32)
    pr = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0]], dtype=torch.float32)
    c, s = np.cos(0.3), np.sin(0.3)
    mv1 = torch.tensor([[c, -s, 0, 0.1], [s, c, 0, -0.05], [0, 0, 1, 0.0], [0, 0, 0, 1]], dtype=torch.float32)
    mv = torch.stack((torch.eye(4), mv1))
    proj = torch.stack((pr, pr * 1.5))
    pos, neg = cgr.clamp_masks(verts, mv, proj)
    assert pos[0].any() and neg[0].any()
    gen = torch.Generator().manual_seed(3)
    g_ndc, g_img, g_aa = (torch.randn(s, generator=gen) for s in ((2, 8, 3), (2, 8, 2), (2, 7, 3, 2)))
    d = "cuda"
    # faces share vertices: the aa route's scatter is not bit-reproducible
    check_prep(verts.to(d), faces.to(d), mv.to(d), proj.to(d), 16, 12, g_ndc.to(d), g_img.to(d), g_aa.to(d), False)


def test_prep_camera_grads_empty_and_invisible():
    d = "cuda"
    mv = torch.eye(4, device=d)[None].repeat(2, 1, 1)
    z3, zf = torch.zeros((0, 3), device=d), torch.zeros((0, 3), dtype=torch.int32, device=d)
    # P = 0 (and F = 0)
    gv, gm, gp = _C.prepare_faces_backward(z3, zf, mv, mv, 8, 8, need_camera=True)
    assert tuple(gv.shape) == (0, 3) and tuple(gm.shape) == (2, 4, 4) and tuple(gp.shape) == (2, 4, 4)
    assert not gm.any() and not gp.any()
    # F = 0 with vertices: the aa route has no corners; ndc still counts
    sc = scenes.triangle_soup(32, 32, 20, scenes.SEED_BASE + 7, num_cams=2).to(d)
    P = sc.verts.shape[0]
    g_aa0 = torch.zeros((2, 0, 3, 2), device=d)
    _, gm, gp = _C.prepare_faces_backward(sc.verts, zf, sc.mv, sc.proj, 32, 32, g_aa_face_verts=g_aa0, need_camera=True)
    assert not gm.any() and not gp.any()
    # views where nothing is visible: every upstream gradient zero (the op sends zeros), or none at all
    faces = sc.faces.to(torch.int32)
    zeros = dict(g_verts_ndc=torch.zeros((2, P, 3), device=d), g_verts_image=torch.zeros((2, P, 2), device=d),
                 g_aa_face_verts=torch.zeros((2, faces.shape[0], 3, 2), device=d))
    for kw in (zeros, {}):
        gv, gm, gp = _C.prepare_faces_backward(sc.verts, faces, sc.mv, sc.proj, 32, 32, need_camera=True, **kw)
        assert gm is not None and gp is not None and tuple(gm.shape) == (2, 4, 4)
        assert not gm.any() and not gp.any() and not gv.any()


# ---- module level -------------------------------------------------------------------------------------------------------
W, H, F = 112, 72, 900


@pytest.fixture(scope="module")
def soup():
    return mixed_orientation(scenes.triangle_soup(W, H, F, scenes.SEED_BASE + 71, num_cams=3, shared_verts=True)).to("cuda")


def render_grads(sc, fused, idx=(0, 1), pm=((0, 0), (0, 0)), pw=W, ph=H, temp=1.0, analytic=False, tfi=None, verts_grad=True,
                 steps=1):
    """One (or more) Renderer.forward + backward with cameras that require grad from construction on -> (mv.grad, proj.grad,
    verts.grad) of the last step."""
    mv, proj = sc.mv.clone().requires_grad_(True), sc.proj.clone().requires_grad_(True)
    r = dm2.Renderer(mv, proj, W, H, "cuda", fused_prep=fused, analytic_rays=analytic, tables_from_image=tfi)
    B = len(idx)
    gen = torch.Generator().manual_seed(17)
    gc, gd = torch.randn((B, ph, pw, 3), generator=gen).cuda(), torch.randn((B, ph, pw), generator=gen).cuda()
    intense = sc.faces_intense[[0] * B] if sc.faces_intense.shape[0] < B else sc.faces_intense[:B]
    for _ in range(steps):
        mv.grad = proj.grad = None
        verts = sc.verts.clone().requires_grad_(verts_grad)
        color, depth = r(list(idx), torch.tensor(pm, dtype=torch.int64, device="cuda"), pw, ph, verts, sc.faces, sc.verts_color,
                         sc.faces_opacity, intense, sc.background, aa_temperature=temp)
        torch.autograd.backward([color, depth], [gc, gd])
    torch.cuda.synchronize()
    assert mv.grad is not None and proj.grad is not None
    return mv.grad.cpu().numpy(), proj.grad.cpu().numpy(), verts.grad


VARIANTS = [
    dict(tfi=True, routed=True),
    dict(tfi=False, routed=True),
    dict(tfi=False, routed=False),
    dict(tfi=True, routed=True, analytic=True),
    dict(tfi=False, routed=False, analytic=True),
    dict(tfi=True, routed=True, temp=0.0),
    dict(tfi=False, routed=False, temp=0.0),
    dict(tfi=True, routed=True, idx=(2, 0, 2), pm=((8, 4), (0, 0), (16, 8)), pw=96, ph=64),
    dict(tfi=False, routed=False, idx=(2, 0, 2), pm=((8, 4), (0, 0), (16, 8)), pw=96, ph=64),
]


@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: "-".join(f"{k}={v[k]}" for k in v))
def test_renderer_camera_grads_vs_torch_prep(soup, monkeypatch, v):
    kw = {k: v[k] for k in ("idx", "pm", "pw", "ph", "temp", "analytic") if k in v}
    monkeypatch.setattr(dm2, "_FUSED_AA_GRAD", v["routed"])
    gm_f, gp_f, _ = render_grads(soup, True, tfi=v["tfi"], **kw)
    gm_t, gp_t, _ = render_grads(soup, False, **kw)
    assert np.abs(gm_t).max() > 0 and np.abs(gp_t).max() > 0
    if "idx" in kw:
        assert np.abs(gm_f[2]).max() > 0 and np.abs(gm_f[0]).max() > 0 and not gm_f[1].any()
    assert rel(gm_f, gm_t) <= 1e-3 and rel(gp_f, gp_t) <= 1e-3


@pytest.mark.parametrize("tfi,routed", [(True, True), (False, True), (False, False)])
def test_renderer_camera_grads_tight_vs_yardstick(soup, monkeypatch, tfi, routed):
    """The camera gradient Renderer hands back equals the yardstick's for the upstream gradients the op actually sent."""
    monkeypatch.setattr(dm2, "_FUSED_AA_GRAD", routed)
    seen = {}

    def spy(real, name):
        def f(verts, faces, mv, proj, width, height):
            outs = real(verts, faces, mv, proj, width, height)
            seen.update(name=name, verts=verts.detach(), faces=faces, mv=mv.detach(), proj=proj.detach(), tabs=outs)
            for i, key in ((0, "g_ndc"), (1, "g_image"), (2, "g_aa")):
                if i < len(outs) and outs[i].requires_grad:
                    outs[i].register_hook(lambda g, key=key: None if g is None else seen.__setitem__(key, g.detach().clone()))
            return outs
        return f

    monkeypatch.setattr(prep, "project", spy(prep.project, "project"))
    monkeypatch.setattr(prep, "prepare", spy(prep.prepare, "prepare"))
    idx = (2, 0, 2)
    gm, gp, _ = render_grads(soup, True, tfi=tfi, idx=idx, pm=((8, 4), (0, 0), (16, 8)), pw=96, ph=64)
    assert seen["name"] == ("project" if tfi and routed else "prepare")
    assert ("g_aa" in seen) == (not routed)
    t = seen["tabs"]
    ref = cgr.camera_grads(seen["verts"], seen["mv"], seen["proj"], W, H, g_ndc=seen.get("g_ndc"), g_image=seen.get("g_image"),
                           g_aa=seen.get("g_aa"), faces=seen["faces"], aa_face_verts=t[2] if len(t) > 2 else None,
                           verts_image=t[1])
    ref_mv, ref_proj = np.zeros((3, 4, 4)), np.zeros((3, 4, 4))
    for i, b in enumerate(idx):
        ref_mv[b] += ref["mv"][i]
        ref_proj[b] += ref["proj"][i]
    assert cgr.rel_to_max(gm, ref_mv) <= BAR and cgr.rel_to_max(gp, ref_proj) <= BAR


@pytest.mark.parametrize("tfi", [True, False])
def test_renderer_camera_only_step(soup, tfi):
    """Camera refinement with fixed geometry: verts without grad -> mv.grad right, verts.grad None; a second step works (the
    rays built at construction hold no autograd graph)."""
    gm_f, gp_f, gv = render_grads(soup, True, tfi=tfi, verts_grad=False, steps=2)
    assert gv is None
    gm_t, gp_t, _ = render_grads(soup, False, verts_grad=False, steps=2)
    assert rel(gm_f, gm_t) <= 1e-3 and rel(gp_f, gp_t) <= 1e-3


def test_camera_grad_off_launches_todays_kernels(soup, monkeypatch):
    """Cameras without grad: the prep backward is the verts-only call."""
    calls = []
    real = _C.prepare_faces_backward

    def spy(*a, **k):
        calls.append(k.get("need_camera", False))
        return real(*a, **k)

    monkeypatch.setattr(_C, "prepare_faces_backward", spy)
    r = dm2.Renderer(soup.mv, soup.proj, W, H, "cuda", fused_prep=True, tables_from_image=False)
    monkeypatch.setattr(dm2, "_FUSED_AA_GRAD", False)
    verts = soup.verts.clone().requires_grad_(True)
    color, depth = r([0, 1], torch.zeros((2, 2), dtype=torch.int64, device="cuda"), W, H, verts, soup.faces, soup.verts_color,
                     soup.faces_opacity, soup.faces_intense[:2], soup.background)
    (color.sum() + depth.sum()).backward()
    assert calls == [False] and verts.grad is not None


@pytest.mark.parametrize("analytic", [False, True])
def test_layered_render_camera_grads(analytic):
    Wl, Hl, bidx = 96, 80, [1, 0]
    ts = scenes.tet_lattice(Wl, Hl, 5, scenes.SEED_BASE + 72, num_cams=2).to("cuda")
    gen = torch.Generator().manual_seed(8)
    P, Fl = ts.verts.shape[0], ts.faces.shape[0]
    color_p = torch.rand((P, 3), generator=gen).cuda()
    opac = (0.2 + 0.7 * torch.rand((Fl,), generator=gen)).cuda()
    intense = torch.rand((2, Fl), generator=gen).cuda()
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    wc, wd = torch.randn((2, Hl, Wl, 3), generator=gen).cuda(), torch.randn((2, Hl, Wl), generator=gen).cuda()
    with torch.no_grad():
        layers, _ = dm2.LayeredRenderer(ts.mv, ts.proj, Wl, Hl, "cuda").generate(bidx, ts.verts, ts.faces, ts.tets, ts.face_tets,
                                                                                 ts.tet_faces, ts.faces_existence, 4)
    res = []
    for fused in (True, False):
        mv, proj = ts.mv.clone().requires_grad_(True), ts.proj.clone().requires_grad_(True)
        lr = dm2.LayeredRenderer(mv, proj, Wl, Hl, "cuda", fused_prep=fused, analytic_rays=analytic)
        verts = ts.verts.clone().requires_grad_(True)
        color, depth = lr.render(bidx, layers, verts, ts.faces, color_p, opac, intense, bg)
        ((color * wc).sum() + (depth * wd).sum()).backward()
        assert mv.grad is not None and proj.grad is not None
        res.append((mv.grad.cpu().numpy(), proj.grad.cpu().numpy()))
    (gm_f, gp_f), (gm_t, gp_t) = res
    assert np.abs(gm_t).max() > 0
    assert rel(gm_f, gm_t) <= 1e-3 and rel(gp_f, gp_t) <= 1e-3
