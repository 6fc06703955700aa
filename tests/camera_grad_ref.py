"""Yardstick of the camera-matrix gradients of the host prep (dm2_prepare_faces_backward_camera): float64 torch autograd of
``Renderer.compute_verts_ndc_image`` (reference __init__.py:239-262) w.r.t. mv, proj (and verts).

The |w| clamp decision is taken from the fp32 projection, as the kernels and the reference's fp32 run take it; everything
after is float64.  The upstream gradients are those of verts_ndc (B,P,3), verts_image (B,P,2) and aa_face_verts (B,F,3,2);
the last is taken back to the vertices' image coordinates through the CCW un-permutation of ``util.scatter_aa_grad_to_verts``.
"""
import numpy as np
import torch

from util import scatter_aa_grad_to_verts

W_EPS = 1e-4


def _np(t, dtype=None):
    a = torch.as_tensor(t).detach().cpu().numpy() if not isinstance(t, np.ndarray) else t
    return a if dtype is None else np.asarray(a, dtype=dtype)


def clamp_masks(verts, mv, proj):
    """(pos, neg) (B,P) bool: where the fp32 projection's w lies in [0, 1e-4) / (-1e-4, 0) (its |w| clamp fires)."""
    v, m, p = (torch.as_tensor(_np(t), dtype=torch.float32) for t in (verts, mv, proj))
    hom = torch.cat((v, torch.ones_like(v[:, :1])), dim=-1)
    w = torch.matmul(torch.matmul(hom, m.transpose(1, 2)), p.transpose(1, 2))[..., 3]
    return (w >= 0) & (w < W_EPS), (w < 0) & (w > -W_EPS)


def project64(verts, mv, proj, width, height, pos, neg):
    """float64 projection with a FIXED clamp mask: -> verts_ndc (B,P,3), verts_image (B,P,2)."""
    hom = torch.cat((verts, torch.ones_like(verts[:, :1])), dim=-1)
    clip = torch.matmul(torch.matmul(hom, mv.transpose(1, 2)), proj.transpose(1, 2))
    w = clip[..., 3]
    w = torch.where(pos, torch.full_like(w, W_EPS), w)
    w = torch.where(neg, torch.full_like(w, -W_EPS), w)
    ndc = clip[..., :3] / w[..., None]
    half = (ndc[..., :2] + 1) * 0.5
    image = torch.stack((half[..., 0] * width, half[..., 1] * height), dim=-1)
    return ndc, image


def upstream_image_grad(g_image=None, g_aa=None, faces=None, aa_face_verts=None, verts_image=None):
    """g_image + the per-vertex sum of g_aa's corners (CCW reorder undone), float64 numpy (B,P,2), or None."""
    out = None
    if g_image is not None:
        out = _np(g_image, np.float64).copy()
    if g_aa is not None:
        s = scatter_aa_grad_to_verts(_np(g_aa), _np(aa_face_verts), _np(verts_image), _np(faces))
        out = s if out is None else out + s
    return out


def camera_grads(verts, mv, proj, width, height, g_ndc=None, g_image=None, g_aa=None, faces=None, aa_face_verts=None,
                 verts_image=None):
    """-> dict(mv=(B,4,4), proj=(B,4,4), verts=(P,3)) float64 numpy: the gradients of
    sum(g_ndc * verts_ndc) + sum(g_image_total * verts_image), g_image_total = g_image + g_aa taken to the vertices.
    aa_face_verts / verts_image: the fp32 tables the prep built (they decide the CCW un-permutation of g_aa)."""
    f64 = torch.float64
    v = torch.as_tensor(_np(verts, np.float64)).clone().requires_grad_(True)
    m = torch.as_tensor(_np(mv, np.float64)).clone().requires_grad_(True)
    p = torch.as_tensor(_np(proj, np.float64)).clone().requires_grad_(True)
    pos, neg = clamp_masks(verts, mv, proj)
    ndc, image = project64(v, m, p, width, height, pos, neg)
    gi = upstream_image_grad(g_image, g_aa, faces, aa_face_verts, verts_image)
    outs, grads = [], []
    if g_ndc is not None:
        outs.append(ndc)
        grads.append(torch.as_tensor(_np(g_ndc, np.float64)))
    if gi is not None:
        outs.append(image)
        grads.append(torch.as_tensor(gi, dtype=f64))
    if not outs:
        z = np.zeros
        return dict(mv=z(tuple(m.shape)), proj=z(tuple(p.shape)), verts=z(tuple(v.shape)))
    gv, gm, gp = torch.autograd.grad(outs, [v, m, p], grads, allow_unused=True)
    fix = lambda g, t: np.zeros(tuple(t.shape)) if g is None else g.numpy()      # noqa: E731
    return dict(mv=fix(gm, m), proj=fix(gp, p), verts=fix(gv, v))


def rel_to_max(got, ref):
    """max |got - ref| / max |ref| (the bar of the camera gradients: 1e-5 of the largest entry)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))
