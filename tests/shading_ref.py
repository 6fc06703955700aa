"""Restatement of Renderer.shading_vectors (include/dm2_hip.h: dm2_shading_vectors_window) in numpy / torch.

  forward32(layers, t, normals, ray_o, ray_d)   float32, every multiply and add rounded separately, in the contract's order: the
                                                kernel must give these bits.  ray_o, ray_d (B,H,W,3): the rays of the slots' pixels
  grads64(...)                                  (dL/dt, dL/dnormals, sabs_t, sabs_n) in float64 by autograd through the forward's
                                                formulas (not through the closed form the kernel uses), with the abs-evaluated sums
                                                of the closed form's terms
Contract: a slot is empty when its id is negative or t is not finite: zeros, no gradient.  position = ro + t * rd; view = -rd;
nl = sqrt((nx nx + ny ny) + nz nz); where nl is zero or not finite normal = reflection = 0; else normal = n / nl,
c = (normal.x view.x + normal.y view.y) + normal.z view.z, reflection = (2 c) normal - view."""
import numpy as np
import torch

f32 = np.float32


def forward32(layers, t, normals, ray_o, ray_d):
    layers, t = np.asarray(layers), np.asarray(t, f32)
    ro, rd = np.asarray(ray_o, f32)[:, :, :, None, :], np.asarray(ray_d, f32)[:, :, :, None, :]
    live = (layers >= 0) & np.isfinite(t)
    with np.errstate(all="ignore"):
        pos = (ro + (t[..., None] * rd).astype(f32)).astype(f32)
        view = np.broadcast_to(-rd, pos.shape).astype(f32)
        pos = np.where(live[..., None], pos, f32(0)).astype(f32)
        view = np.where(live[..., None], view, f32(0)).astype(f32)
        if normals is None:
            return pos, view
        n = np.asarray(normals, f32)
        nl = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).astype(f32)
        good = live & np.isfinite(nl) & (nl != 0)
        nrm = (n / np.where(good, nl, f32(1))[..., None]).astype(f32)
        c = (nrm[..., 0] * view[..., 0] + nrm[..., 1] * view[..., 1]) + nrm[..., 2] * view[..., 2]
        refl = ((f32(2.0) * c)[..., None] * nrm - view).astype(f32)
        nrm = np.where(good[..., None], nrm, f32(0)).astype(f32)
        refl = np.where(good[..., None], refl, f32(0)).astype(f32)
    return pos, view, nrm, refl


def _good64(layers, t, normals):
    live = (np.asarray(layers) >= 0) & np.isfinite(np.asarray(t, f32))
    if normals is None:
        return live, None
    n = np.asarray(normals, f32)
    with np.errstate(all="ignore"):
        nl = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).astype(f32)    # the kernel's own test
    return live, live & np.isfinite(nl) & (nl != 0)


def _clean(x):
    """float64 copy with the non-finite entries replaced (for autograd's sake only: their slots are empty / zero by _good64)."""
    return torch.from_numpy(np.where(np.isfinite(np.asarray(x, f32)), np.asarray(x, np.float64), 0.0))


def _loss(tt, nn, live, good, ray_o, ray_d, g_pos, g_nrm, g_refl):
    ro = torch.from_numpy(np.asarray(ray_o, np.float64))[:, :, :, None, :]
    rd = torch.from_numpy(np.asarray(ray_d, np.float64))[:, :, :, None, :]
    lv = torch.from_numpy(live)
    total = torch.zeros((), dtype=torch.float64)
    if g_pos is not None:
        pos = ro + tt[..., None] * rd
        total = total + (torch.where(lv[..., None], pos, torch.zeros_like(pos)) * torch.from_numpy(np.asarray(g_pos, np.float64))).sum()
    if nn is not None and (g_nrm is not None or g_refl is not None):
        gd = torch.from_numpy(good)
        nsafe = torch.where(gd[..., None], nn, torch.ones_like(nn))
        nrm = nsafe / nsafe.norm(dim=-1, keepdim=True)
        view = (-rd).expand_as(nrm)
        refl = 2.0 * (nrm * view).sum(-1, keepdim=True) * nrm - view
        for out, g in ((nrm, g_nrm), (refl, g_refl)):
            if g is not None:
                total = total + (torch.where(gd[..., None], out, torch.zeros_like(out)) * torch.from_numpy(np.asarray(g, np.float64))).sum()
    return total


def loss64(layers, t, normals, ray_o, ray_d, g_pos, g_nrm, g_refl, t64=None, n64=None):
    """sum of the outputs times their upstream gradients (None: left out), float64; which slots are empty is decided on the
    float32 inputs, as the kernel decides it.  t64 / n64: float64 values to evaluate at instead (central differences)."""
    live, good = _good64(layers, t, normals)
    tt = _clean(t) if t64 is None else torch.from_numpy(t64)
    nn = None if normals is None else (_clean(normals) if n64 is None else torch.from_numpy(n64))
    return float(_loss(tt, nn, live, good, ray_o, ray_d, g_pos, g_nrm, g_refl))


def grads64(layers, t, normals, ray_o, ray_d, g_pos, g_nrm, g_refl):
    """-> (dL/dt (B,H,W,L), dL/dnormals (B,H,W,L,3) or None, sabs_t, sabs_n): the gradients by float64 autograd, and per element
    the closed form evaluated on absolute values (what 8 eps32 times it bounds is the rounding of any fp32 evaluation)."""
    live, good = _good64(layers, t, normals)
    tt = _clean(t).requires_grad_(True)
    nn = None if normals is None else _clean(normals).requires_grad_(True)
    rd64 = np.asarray(ray_d, np.float64)[:, :, :, None, :]
    total = _loss(tt, nn, live, good, ray_o, ray_d, g_pos, g_nrm, g_refl)
    if total.requires_grad:
        total.backward()
    dt = tt.grad.numpy() if tt.grad is not None else np.zeros(live.shape)
    dn = None if nn is None else (nn.grad.numpy() if nn.grad is not None else np.zeros(live.shape + (3,)))
    # abs-evaluated closed form
    sabs_t = np.zeros(live.shape)
    if g_pos is not None:
        sabs_t = np.where(live, (np.abs(np.asarray(g_pos, np.float64)) * np.abs(rd64)).sum(-1), 0.0)
    sabs_n = None
    if normals is not None:
        n64 = np.where(good[..., None], np.asarray(normals, np.float64), 1.0)
        nl = np.sqrt((n64 * n64).sum(-1, keepdims=True))
        a = np.abs(n64 / nl)
        v = np.broadcast_to(np.abs(rd64), a.shape)
        c = (a * v).sum(-1, keepdims=True)
        gn = np.zeros_like(a) if g_nrm is None else np.abs(np.asarray(g_nrm, np.float64))
        gr = np.zeros_like(a) if g_refl is None else np.abs(np.asarray(g_refl, np.float64))
        G = gn + 2.0 * c * gr + 2.0 * (gr * a).sum(-1, keepdims=True) * v
        sabs_n = np.where(good[..., None], (G + a * (a * G).sum(-1, keepdims=True)) / nl, 0.0)
    return dt, dn, sabs_t, sabs_n
