"""CPU checks of the camera-gradient yardstick (camera_grad_ref.py) that the GPU tests hold the fused prep's
dm2_prepare_faces_backward_camera to: float64 finite differences of the projection, and torch autograd of the
reference-shaped host prep (Renderer.compute_verts_ndc_image + Triangles) -- clamped vertices and repeated views included."""
import numpy as np
import torch

import camera_grad_ref as cgr
import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import scenes
from dmesh2_renderer_amd.pyrenderer import Triangles


def clamped_scene(num_cams=3, seed=61):
    """A small soup with three cameras, plus vertices placed on each camera's w ~ 0 plane (|w| < 1e-4 both signs, and 0)."""
    W, H = 64, 48
    sc = scenes.triangle_soup(W, H, 60, scenes.SEED_BASE + seed, num_cams=num_cams, shared_verts=True)
    verts, mv, proj = sc.verts.clone(), sc.mv.clone(), sc.proj.clone()
    extra = []
    for b in range(num_cams):
        inv = torch.inverse(mv[b].double())
        wrow = proj[b, 3].double()                          # w = wrow . (mv hom): solve for view-space points with w ~ 0
        for w_target, x in ((0.5e-4, 0.2), (-0.5e-4, -0.1), (0.0, 0.05)):
            # clip w = wrow . t; take t = (x, 0.1, z, 1) and solve wrow . t = w_target for z
            z = (w_target - (wrow[0] * x + wrow[1] * 0.1 + wrow[3])) / wrow[2]
            t = torch.tensor([x, 0.1, float(z), 1.0], dtype=torch.float64)
            extra.append((inv @ t)[:3].float())
    P0 = verts.shape[0]
    verts = torch.cat((verts, torch.stack(extra)), dim=0)
    n = len(extra)
    faces = torch.cat((sc.faces, torch.tensor([[P0 + i, P0 + (i + 1) % n, 0] for i in range(n)], dtype=sc.faces.dtype)), dim=0)
    return W, H, verts, faces, mv, proj


def test_clamped_scene_clamps():
    W, H, verts, faces, mv, proj = clamped_scene()
    pos, neg = cgr.clamp_masks(verts, mv, proj)
    assert pos.any() and neg.any()


def test_yardstick_vs_finite_differences():
    W, H, verts, faces, mv, proj = clamped_scene()
    B, P = mv.shape[0], verts.shape[0]
    gen = torch.Generator().manual_seed(5)
    g_ndc, g_img = torch.randn((B, P, 3), generator=gen), torch.randn((B, P, 2), generator=gen)
    ref = cgr.camera_grads(verts, mv, proj, W, H, g_ndc=g_ndc, g_image=g_img)
    pos, neg = cgr.clamp_masks(verts, mv, proj)
    v64, m64, p64 = verts.double(), mv.double(), proj.double()
    gn64, gi64 = g_ndc.double(), g_img.double()

    def loss(m, p):
        ndc, image = cgr.project64(v64, m, p, W, H, pos, neg)
        return float((ndc * gn64).sum() + (image * gi64).sum())

    h = 1e-6
    fd_mv, fd_proj = np.zeros((B, 4, 4)), np.zeros((B, 4, 4))
    for b in range(B):
        for j in range(4):
            for k in range(4):
                for fd, which in ((fd_mv, 0), (fd_proj, 1)):
                    a, c = m64.clone(), p64.clone()
                    t = a if which == 0 else c
                    t[b, j, k] += h
                    up = loss(a, c)
                    t[b, j, k] -= 2 * h
                    fd[b, j, k] = (up - loss(a, c)) / (2 * h)
    assert cgr.rel_to_max(ref["mv"], fd_mv) <= 1e-5
    assert cgr.rel_to_max(ref["proj"], fd_proj) <= 1e-5


def test_yardstick_vs_reference_torch_path():
    """Every upstream route, clamped vertices, repeated views: the reference-shaped fp32 torch path's mv.grad / proj.grad
    (autograd through the index of the selected cameras, as Renderer.forward takes them) against the fp64 yardstick."""
    W, H, verts, faces, mv_all, proj_all = clamped_scene()
    idx = [2, 0, 2]
    B, P, F = len(idx), verts.shape[0], faces.shape[0]
    gen = torch.Generator().manual_seed(6)
    g_ndc, g_img, g_aa = (torch.randn(s, generator=gen) for s in ((B, P, 3), (B, P, 2), (B, F, 3, 2)))
    r = dm2.Renderer.__new__(dm2.Renderer)
    r.width, r.height = W, H
    for route in ("ndc", "image", "aa", "all"):
        m_all, p_all = mv_all.clone().requires_grad_(True), proj_all.clone().requires_grad_(True)
        ndc, image = dm2.Renderer.compute_verts_ndc_image(r, verts, m_all[idx], p_all[idx])
        corners = image[:, faces.flatten()].view(-1, 3, 2)
        tri = Triangles(corners[:, 0], corners[:, 1], corners[:, 2])
        aav = tri.verts.reshape(B, F, 3, 2)
        outs, grads = [], []
        if route in ("ndc", "all"):
            outs.append(ndc); grads.append(g_ndc)
        if route in ("image", "all"):
            outs.append(image); grads.append(g_img)
        if route in ("aa", "all"):
            outs.append(aav); grads.append(g_aa)
        torch.autograd.backward(outs, grads)
        kw = dict(g_ndc=g_ndc if route in ("ndc", "all") else None, g_image=g_img if route in ("image", "all") else None,
                  g_aa=g_aa if route in ("aa", "all") else None, faces=faces, aa_face_verts=aav.detach(), verts_image=image.detach())
        ref = cgr.camera_grads(verts, mv_all[idx], proj_all[idx], W, H, **kw)
        ref_mv, ref_proj = np.zeros((3, 4, 4)), np.zeros((3, 4, 4))
        for i, b in enumerate(idx):                          # autograd's index backward sums the repeated view
            ref_mv[b] += ref["mv"][i]
            ref_proj[b] += ref["proj"][i]
        assert np.abs(ref_mv[1]).max() == 0 and np.abs(ref_mv[2]).max() > 0
        assert cgr.rel_to_max(m_all.grad.numpy(), ref_mv) <= 1e-4, route
        assert cgr.rel_to_max(p_all.grad.numpy(), ref_proj) <= 1e-4, route


def test_yardstick_without_upstream_is_zero():
    W, H, verts, faces, mv, proj = clamped_scene(num_cams=1)
    ref = cgr.camera_grads(verts, mv, proj, W, H)
    assert ref["mv"].shape == (1, 4, 4) and not ref["mv"].any() and not ref["proj"].any()
