"""The general cameras of tests/cameras.py and what the references see under them (no GPU).

* the matrices and scenes are what cameras.py claims: no zero where none is promised, an asymmetric rotation, both
  windings in every view, w = 1 for the un-projected near point, views that render, a grazing view that clamps;
* the oracle's prep and closed-form rays equal plain numpy float32 restatements of the same formulas bit for bit, and stay
  within a worked-out rounding bound of float64 numpy of the same formulas;
* the oracle's prep backward and the camera-gradient yardstick agree with float64 torch autograd of the host twin;
* teeth: a reassociated sum or a transposed rotation block changes NO bit under ``scenes.camera`` and a large share of the
  values under the general cameras -- the gap tests/test_gpu_general_cameras.py closes.
"""
import numpy as np
import pytest
import torch

import cameras
import camera_grad_ref as cgr
from util import capture_forward_args, scenes, to_numpy_args

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd.pyrenderer import Triangles
from oracle import cpu as orc

W, H, F = 96, 72, 600
SEED = scenes.SEED_BASE + 5
EPS32 = 2.0 ** -24            # unit roundoff of float32
AUTOGRAD_BAR = 1e-5           # test_oracle_prep.py's bar of the oracle's fp32 backward against torch autograd
GPU_FP64_BAR = 1e-5           # test_gpu_general_cameras.py's bar of d(verts) against float64
RAY_BOUND = 3e-6              # no component of a float32 ray direction is further from float64 (the bound of test_oracle_rays_equal_numpy)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def soup():
    return cameras.reposed_soup(W, H, F, SEED, 3, shared_verts=True)


@pytest.fixture(scope="module")
def grazing():
    return cameras.grazing_soup(W, H, F, SEED, 2, shared_verts=True)


@pytest.fixture(scope="module")
def plain():
    return scenes.triangle_soup(W, H, F, SEED, shared_verts=True)


# ---- numpy restatements ----------------------------------------------------------------------------------------------------
def sum4(terms, order="left"):
    a, b, c, d = terms
    return ((a + b) + c) + d if order == "left" else a + (b + (c + d))


def project_np(verts, mv, proj, width, height, dtype=np.float32, order="left", clamp=None):
    """k_project's formulas on numpy arrays of ``dtype``: both 4x4 products summed k = 0..3 (``order`` "right": a + (b + (c +
    d)) instead), the |w| clamp (``clamp`` = (pos, neg) masks: decisions given instead of taken), NDC, the image mapping.
    -> verts_ndc (B,P,3), verts_image (B,P,2), w (B,P), A_c (B,P,3), A_w (B,P): the sums of the absolute values of every
    product that enters a clip coordinate / w (float64; what a rounding bound scales with)."""
    f = dtype
    v, m, p = np.asarray(verts, f), np.asarray(mv, f), np.asarray(proj, f)
    hom = [v[None, :, 0], v[None, :, 1], v[None, :, 2], f(1.0)]
    t = [sum4([hom[k] * m[:, j, k][:, None] for k in range(4)], order) for j in range(4)]
    c = [sum4([t[k] * p[:, j, k][:, None] for k in range(4)], order) for j in range(4)]
    w = c[3]
    pos, neg = ((w >= 0) & (w < f(cameras.W_EPS)), (w < 0) & (w > f(-cameras.W_EPS))) if clamp is None else clamp
    w = np.where(pos, f(cameras.W_EPS), np.where(neg, f(-cameras.W_EPS), w)).astype(f)
    ndc = np.stack([c[0] / w, c[1] / w, c[2] / w], axis=-1)
    image = np.stack([((ndc[..., 0] + f(1.0)) * f(0.5)) * f(width), ((ndc[..., 1] + f(1.0)) * f(0.5)) * f(height)], axis=-1)
    assert ndc.dtype == f and image.dtype == f
    habs = np.concatenate((np.abs(np.asarray(verts, np.float64)), np.ones((v.shape[0], 1))), axis=1)
    A = np.einsum("bjk,bkl,pl->bpj", np.abs(np.asarray(proj, np.float64)), np.abs(np.asarray(mv, np.float64)), habs)
    return ndc, image, w, A[..., :3], A[..., 3]


def rays_np(imv, ipr, width, height, dtype=np.float32, order="left"):
    """analytic_ray's formulas (csrc/dm2_device_math.h) on numpy arrays of ``dtype`` -> ray_o, ray_d (B,H,W,3), A (B,H,W,3):
    the sum of the absolute values of every product that enters the un-normalised target."""
    f = dtype
    imv, ipr = np.asarray(imv, f), np.asarray(ipr, f)
    B = imv.shape[0]
    hx = ((np.arange(width, dtype=f) + f(0.5)) / f(width) * f(2.0)) - f(1.0)
    hy = ((np.arange(height, dtype=f) + f(0.5)) / f(height) * f(2.0)) - f(1.0)
    h = [np.broadcast_to(hx[None, None, :], (B, height, width)), np.broadcast_to(hy[None, :, None], (B, height, width)), f(-1.0), f(1.0)]
    e = lambda m, j, k: m[:, j, k][:, None, None]                                  # noqa: E731
    v = [sum4([h[k] * e(ipr, j, k) for k in range(4)], order) for j in range(4)]
    w = [sum4([v[k] * e(imv, j, k) for k in range(4)], order) for j in range(3)]
    ro = np.stack([np.broadcast_to(e(imv, j, 3), (B, height, width)) for j in range(3)], axis=-1)
    d = np.stack([w[j] - ro[..., j] for j in range(3)], axis=-1)
    ln = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + f(1e-6)
    rd = d / ln[..., None]
    assert rd.dtype == f
    habs = np.stack([np.abs(h[0]).astype(np.float64), np.abs(h[1]).astype(np.float64), np.ones((B, height, width)),
                     np.ones((B, height, width))], axis=-1)
    A = np.einsum("bjk,bkl,bhwl->bhwj", np.abs(imv[:, :3].astype(np.float64)), np.abs(ipr.astype(np.float64)), habs)
    return np.ascontiguousarray(ro), np.ascontiguousarray(rd), A, ln


def transposed_rotation(m):
    m = np.array(m, copy=True)
    m[..., :3, :3] = np.swapaxes(m[..., :3, :3], -1, -2)
    return m


def inverses(sc):
    """inv(mv), inv(proj) in float32, as Renderer(analytic_rays=True) hands them to the kernels."""
    return torch.inverse(sc.mv).numpy(), torch.inverse(sc.proj).numpy()


# ---- the matrices and the scenes ---------------------------------------------------------------------------------------
def test_matrix_properties(soup, grazing):
    for sc, dense in ((soup, False), (grazing, True)):
        mv, proj = sc.mv.numpy(), sc.proj.numpy()
        assert (mv[:, :3, :4] != 0).all()
        R = mv[:, :3, :3]
        assert (np.abs(R - np.swapaxes(R, 1, 2)).max(axis=(1, 2)) > 0.1).all()
        assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-6
        assert (proj[:, :3 if dense else 2] != 0).all()
        assert (proj[:, 0, 2] != 0).all() and (proj[:, 1, 2] != 0).all()
        assert np.array_equal(proj[:, 3], np.broadcast_to(np.float32([0, 0, -1, 0]), (len(proj), 4)))      # w unchanged
        # no two views share a matrix, pixels are not square
        assert len({m.tobytes() for m in mv}) == len(mv) and len({p.tobytes() for p in proj}) == len(proj)
        assert (np.abs(proj[:, 0, 0] * sc.width - proj[:, 1, 1] * sc.height) > 0.01 * sc.height).all()
    assert (soup.proj.numpy()[:, 2, :2] == 0).all() and (grazing.proj.numpy()[:, 2] != 0).all()
    assert int((soup.mv[0] != 0).sum()) == 13 and int((grazing.proj[0] != 0).sum()) == 13 and int((soup.proj[0] != 0).sum()) == 11
    # the un-projected near point keeps w = 1 in the rendered variant (rays without a perspective divide are pixel rays)
    ipr = np.linalg.inv(soup.proj.numpy().astype(np.float64)).astype(np.float32)
    for x, y in ((-1, -1), (1, -1), (0.3, 0.7), (1, 1)):
        w = ipr @ np.float32([x, y, -1, 1])
        assert np.abs(w[:, 3] - 1).max() <= 8 * EPS32
    # the closed-form rays agree with the reference-shaped torch rays (Renderer._init_rays)
    r = dm2.Renderer(soup.mv, soup.proj, W, H, "cpu")
    ro, rd = orc.analytic_rays_from_inverse(*inverses(soup), W, H)
    assert np.abs(rd - r.ray_d.numpy()).max() <= 1e-6 and np.abs(ro - r.ray_o.numpy()).max() <= 1e-6


def test_both_windings_in_every_view(soup, grazing):
    for sc in (soup, grazing):
        out = orc.prepare_faces(sc.verts, sc.faces, sc.mv, sc.proj, W, H)
        v1 = out["verts_image"][:, sc.faces.numpy()[:, 1]]
        flipped = np.any(out["verts"][:, :, 1] != v1, axis=-1)              # (B,F): the CCW reorder swapped corners 1 and 2
        assert flipped.any(axis=1).all() and (~flipped).any(axis=1).all()
        assert (flipped.mean(axis=1) > 0.25).all() and (flipped.mean(axis=1) < 0.75).all()


def test_rendered_scenes_render(soup):
    """Conditions on the rendered scenes, on the oracle: every view blends a face in at least half of its pixels at
    temperature 0, lists pairs, and keeps every vertex at w >= 0.5."""
    _, _, w, _, _ = project_np(soup.verts.numpy(), soup.mv.numpy(), soup.proj.numpy(), W, H)
    assert w.min() >= 0.5
    for b in range(3):
        args, _ = capture_forward_args(soup, [b], [[0, 0]], W, H, temp=0.0)
        ref = orc.render_forward_cuda(*to_numpy_args(args), nthreads=orc.max_threads())
        share = float((ref.final_T < 1.0).mean())
        print(f"view {b}: num_rendered {ref.num_rendered}, share of pixels that blend a face {share:.3f}")
        assert ref.num_rendered > 0 and share >= 0.5
    ts = cameras.reposed_lattice(64, 48, 4, scenes.SEED_BASE + 6, 2)
    _, _, w, _, _ = project_np(ts.verts.numpy(), ts.mv.numpy(), ts.proj.numpy(), 64, 48)
    assert w.min() >= 0.5 and (ts.mv.numpy()[:, :3, :4] != 0).all()
    ndc, img = (torch.from_numpy(x) for x in project_np(ts.verts.numpy(), ts.mv.numpy(), ts.proj.numpy(), 64, 48)[:2])
    ro, rd = orc.analytic_rays_from_inverse(*inverses(ts), 64, 48)
    _, cnt = orc.generate_render_layers_cuda(64, 48, ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence,
                                             ndc, img, ro, rd, 4)
    assert ((cnt > 0).mean(axis=(1, 2)) >= 0.5).all()


def test_grazing_view_clamps(grazing):
    pos, neg = cgr.clamp_masks(grazing.verts, grazing.mv, grazing.proj)
    _, image, w, _, _ = project_np(grazing.verts.numpy(), grazing.mv.numpy(), grazing.proj.numpy(), W, H)
    cl = np.abs(w) == np.float32(cameras.W_EPS)
    assert np.array_equal(cl, (pos | neg).numpy())                             # (torch's matmul takes the same decisions)
    assert not cl[:-1].any() and cl[-1].sum() >= 20 and pos[-1].sum() >= 8 and neg[-1].sum() >= 8
    assert (w[-1] < 0).sum() >= 20 and (w[-1] < -cameras.GRAZE_BAND).sum() >= 20
    assert np.abs(w[-1][~cl[-1]]).min() >= cameras.GRAZE_BAND * 0.999
    print(f"grazing view: {cl[-1].sum()} clamped, {(w[-1] < 0).sum()} of {w.shape[1]} vertices with w < 0, "
          f"|verts_image| up to {np.abs(image).max():.3g} px")
    assert np.abs(image).max() > 1e5


# ---- oracle against numpy ------------------------------------------------------------------------------------------------
def ndc_bound(ndc64, w64, A_c, A_w):
    """Rounding bound of the float32 NDC, element-wise: a product-sum of 4 terms carries (1 + 3) roundings a term, two nested
    ones 8, the division one more: |d(c)| <= 9 u A_c, |d(w)| <= 8 u A_w (A: the sum of |products|, u = 2^-24), hence
    |d(c / w)| <= (9 u A_c + |c / w| 8 u A_w) / |w|, to first order; 10 u for both covers the second order."""
    return 10 * EPS32 * (A_c + np.abs(ndc64) * A_w[..., None]) / np.abs(w64)[..., None]


@pytest.mark.parametrize("which", ["soup", "grazing"])
def test_oracle_prep_equals_numpy(which, soup, grazing):
    sc = soup if which == "soup" else grazing
    v, mv, proj = sc.verts.numpy(), sc.mv.numpy(), sc.proj.numpy()
    out = orc.prepare_faces(v, sc.faces, mv, proj, W, H)
    ndc, image, w, A_c, A_w = project_np(v, mv, proj, W, H)
    assert np.array_equal(bits(out["verts_ndc"]), bits(ndc)) and np.array_equal(bits(out["verts_image"]), bits(image))
    # float32 against float64 of the same formulas (the clamp decisions are float32's)
    cl = np.abs(w) == np.float32(cameras.W_EPS)
    n64, i64, w64, _, _ = project_np(v, mv, proj, W, H, np.float64, clamp=(cl & (w > 0), cl & (w < 0)))
    bound = ndc_bound(n64, w64, A_c, A_w)
    err = np.abs(ndc - n64)
    # image = ((n + 1) * 0.5) * W: three more roundings of a value of size |n| + 1
    ibound = (bound[..., :2] + 3 * EPS32 * (np.abs(n64[..., :2]) + 1)) * 0.5 * np.float64([W, H])
    ierr = np.abs(image - i64)
    print(f"{which}: ndc fp32 vs fp64 {rel(ndc, n64):.3g} of the largest entry, worst err / bound {np.max(err / bound):.3f}; "
          f"image {rel(image, i64):.3g}, worst err / bound {np.max(ierr / ibound):.3f}; largest bound / |ndc| "
          f"{np.max(bound / np.maximum(np.abs(n64), 1e-3)):.3g}")
    assert (err <= bound).all() and (ierr <= ibound).all()


def test_oracle_rays_equal_numpy(soup, grazing):
    for sc in (soup, grazing):
        imv, ipr = inverses(sc)
        ro, rd = orc.analytic_rays_from_inverse(imv, ipr, W, H)
        ro32, rd32, A, _ = rays_np(imv, ipr, W, H)
        assert np.array_equal(bits(ro), bits(ro32)) and np.array_equal(bits(rd), bits(rd32))
        ro64, rd64, _, ln = rays_np(imv, ipr, W, H, np.float64)
        # the target's components: 9 roundings a term (two nested 4-term product sums and the subtraction of ray_o), 10 u A
        # with the second order; the length moves by at most |d(target)|_2 plus 3 roundings of its own, the quotient one more
        dd = 10 * EPS32 * A
        bound = (dd + np.linalg.norm(dd, axis=-1, keepdims=True)) / ln[..., None] + 5 * EPS32
        err = np.abs(rd32 - rd64)
        print(f"ray directions fp32 vs fp64: {err.max():.3g} absolute, worst err / bound {np.max(err / bound):.3f}, "
              f"largest bound {bound.max():.3g}")
        assert (err <= bound).all() and bound.max() <= RAY_BOUND and np.array_equal(ro32.astype(np.float64), ro64)


# ---- backward --------------------------------------------------------------------------------------------------------------
def host_twin64(verts, faces, mv, proj):
    """float64 torch of the reference-shaped host prep -> leaves (verts, mv, proj), outputs (ndc, image, aa_face_verts)."""
    leaves = [torch.as_tensor(np.asarray(t, np.float64)).clone().requires_grad_(True) for t in (verts, mv, proj)]
    r = dm2.Renderer.__new__(dm2.Renderer)
    r.width, r.height = W, H
    ndc, image = dm2.Renderer.compute_verts_ndc_image(r, *leaves)
    corners = image[:, torch.as_tensor(np.asarray(faces)).flatten().long()].view(-1, 3, 2)
    tri = Triangles(corners[:, 0], corners[:, 1], corners[:, 2])
    return leaves, (ndc, image, tri.verts.reshape(leaves[1].shape[0], -1, 3, 2))


def upstreams(sc, seed=5):
    B, P, Fc = sc.mv.shape[0], sc.verts.shape[0], sc.faces.shape[0]
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(s, generator=g) for s in ((B, P, 3), (B, P, 2), (B, Fc, 3, 2)))


ROUTES = {"ndc": (0,), "image": (1,), "aa": (2,), "all": (0, 1, 2)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_backward_references_against_float64_autograd(route, soup):
    """The oracle's fp32 prepare_faces_backward within test_oracle_prep.py's 1e-5 of float64 autograd of the host twin, and
    the camera yardstick (float64 itself: another formulation, summation order apart) within 1e-9 of it."""
    gs = upstreams(soup)
    use = ROUTES[route]
    leaves, outs = host_twin64(soup.verts.numpy(), soup.faces.numpy(), soup.mv.numpy(), soup.proj.numpy())
    gv, gm, gp = torch.autograd.grad([outs[i] for i in use], leaves, [gs[i].double() for i in use])
    kw = {("g_ndc", "g_image", "g_aa")[i]: gs[i] for i in use}
    got = orc.prepare_faces_backward(soup.verts, soup.faces, soup.mv, soup.proj, W, H, **kw)
    tabs = orc.prepare_faces(soup.verts, soup.faces, soup.mv, soup.proj, W, H)
    ref = cgr.camera_grads(soup.verts, soup.mv, soup.proj, W, H, faces=soup.faces, aa_face_verts=tabs["verts"],
                           verts_image=tabs["verts_image"], **kw)
    print(f"{route}: oracle fp32 d(verts) {rel(got, gv.numpy()):.3g}; yardstick mv {rel(ref['mv'], gm.numpy()):.3g} "
          f"proj {rel(ref['proj'], gp.numpy()):.3g} verts {rel(ref['verts'], gv.numpy()):.3g}")
    assert rel(got, gv.numpy()) <= AUTOGRAD_BAR
    assert np.abs(gm.numpy()).max() > 0 and np.abs(gp.numpy()).max() > 0
    assert rel(ref["mv"], gm.numpy()) <= 1e-9 and rel(ref["proj"], gp.numpy()) <= 1e-9 and rel(ref["verts"], gv.numpy()) <= 1e-9


@pytest.mark.parametrize("route", list(ROUTES))
def test_oracle_backward_on_the_grazing_view(route, grazing):
    """With the clamp: the yardstick's float64 d(verts) (float32's clamp decisions, fixed) is the reference."""
    gs = upstreams(grazing, 6)
    kw = {("g_ndc", "g_image", "g_aa")[i]: gs[i] for i in ROUTES[route]}
    got = orc.prepare_faces_backward(grazing.verts, grazing.faces, grazing.mv, grazing.proj, W, H, **kw)
    tabs = orc.prepare_faces(grazing.verts, grazing.faces, grazing.mv, grazing.proj, W, H)
    ref = cgr.camera_grads(grazing.verts, grazing.mv, grazing.proj, W, H, faces=grazing.faces, aa_face_verts=tabs["verts"],
                           verts_image=tabs["verts_image"], **kw)
    print(f"grazing {route}: oracle fp32 d(verts) against float64 {rel(got, ref['verts']):.3g}")
    assert rel(got, ref["verts"]) <= AUTOGRAD_BAR


# ---- teeth -----------------------------------------------------------------------------------------------------------------
def test_teeth_projection(plain, soup, grazing):
    """What a kernel with reassociated sums, or one that reads mv's rotation block transposed, would compute."""
    def changed(sc):
        v, mv, proj = sc.verts.numpy(), sc.mv.numpy(), sc.proj.numpy()
        right = project_np(v, mv, proj, W, H)[1]
        reassoc = project_np(v, mv, proj, W, H, order="right")[1]
        transposed = project_np(v, transposed_rotation(mv), proj, W, H)[1]
        return right.size, int((bits(right) != bits(reassoc)).sum()), int((bits(right) != bits(transposed)).sum())
    n, a, t = changed(plain)
    print(f"scenes.camera: reassociation changes {a} of {n} image values, the transposition {t}")
    assert a == 0 and t == 0
    for name, sc in (("reposed_soup", soup), ("grazing_soup", grazing)):
        n, a, t = changed(sc)
        print(f"{name}: reassociation changes {a} of {n} image values, the transposition {t}")
        assert a > 0.1 * n and t > 0.1 * n


def test_teeth_rays(plain, soup):
    def changed(sc):
        imv, ipr = inverses(sc)
        right = rays_np(imv, ipr, W, H)[1]
        reassoc = rays_np(imv, ipr, W, H, order="right")[1]
        transposed = rays_np(transposed_rotation(imv), ipr, W, H)[1]
        return right.size, int((bits(right) != bits(reassoc)).sum()), int((bits(right) != bits(transposed)).sum()), \
            float(np.abs(right - transposed).max())
    n, a, t, _ = changed(plain)
    print(f"scenes.camera: reassociation changes {a} of {n} ray components, the transposition {t}")
    assert a == 0 and t == 0
    n, a, t, dist = changed(soup)
    print(f"reposed_soup: reassociation changes {a} of {n} ray components, the transposition {t} (by up to {dist:.3g})")
    assert a > 0.1 * n and t > 0.1 * n
    # (the GPU tests hold the rays' consumers to the oracle bit for bit; the yardstick here is float32's rounding bound)
    assert dist > 1e3 * RAY_BOUND


def test_teeth_backward(plain, soup):
    """float64 d(verts) with mv's rotation read transposed in the last step (M[0], M[1], M[2] for M[0], M[4], M[8])."""
    def wrong_and_right(sc):
        gs = upstreams(sc, 7)
        right = np.zeros(tuple(sc.verts.shape))
        wrong = np.zeros_like(right)
        for b in range(sc.mv.shape[0]):
            g = cgr.camera_grads(sc.verts, sc.mv[b:b + 1], sc.proj[b:b + 1], W, H, g_ndc=gs[0][b:b + 1], g_image=gs[1][b:b + 1])["verts"]
            R = sc.mv[b, :3, :3].numpy().astype(np.float64)
            right += g                                                   # = g_view @ R
            wrong += g @ np.linalg.inv(R) @ R.T                          # = g_view @ R^T
        return rel(wrong, right)
    assert wrong_and_right(plain) == 0.0
    d = wrong_and_right(soup)
    print(f"reposed_soup: d(verts) with the rotation transposed is {d:.3g} of the largest entry away")
    assert d > 1e3 * GPU_FP64_BAR
