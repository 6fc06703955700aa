"""The mathematics of Renderer.bary_derivatives and its restatement (tests/bary_derivatives_ref.py), without a GPU: the float64
formula against central differences of Moeller-Trumbore, the float32 operation order against float64, empty and degenerate
slots, windows, and the module's surface."""
import numpy as np
import pytest
import torch

import bary_derivatives_ref as bref
import rasterize_ref as rref
from util import rel_linf

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

STEP = 1e-3            # pixels, the central differences' step
_CASES = {}


def case(name, L=3):
    """rasterize_ref.scene(name) with its CPU lists for L layers and the views' camera block."""
    if (name, L) not in _CASES:
        s = rref.scene(name)
        ras = rref.rasterize32(s["W"], s["H"], s["verts"], s["faces"], None, s["verts_ndc"], s["verts_image"], s["ray_o"], s["ray_d"], L)
        _CASES[(name, L)] = dict(s, layers=ras["layers"], cam=bref.camera_block(*bref.scene_cameras(name)))
    return _CASES[(name, L)]


@pytest.mark.parametrize("name", ["soup", "lattice"])
def test_formula_against_central_differences(name):
    """d(u, v)/dX and /dY of the float64 formula against (f(X + h) - f(X - h)) / 2h of float64 Moeller-Trumbore on the rays of
    the fractional positions, h = 1e-3 px.

    Along an axis u is a Moebius function of the position, u = A + B / (Dc + (g.c) x), so the central difference is the
    derivative divided by 1 - q^2, q = h (g.c) / Dc, exactly: the acceptance is |an| q^2 / (1 - q^2) for that, plus the rounding
    of the four evaluations of u (uv64's own bound, over 2h, doubled for the formula's own rounding).  Slots whose pole lies
    within two steps (|q| >= 0.5) are left out; they must be fewer than 1 in 100."""
    c = case(name)
    W, H, rl = c["W"], c["H"], c["layers"]
    B = rl.shape[0]
    dx, dy, p = bref.forward64(rl, c["verts"], c["faces"], c["cam"], W, H, parts=True)
    live = p["live"]
    assert live.sum() > 5000
    X = np.broadcast_to(np.arange(W, dtype=np.float64)[None, None, :], (B, H, W))
    Y = np.broadcast_to(np.arange(H, dtype=np.float64)[None, :, None], (B, H, W))
    worst = 0.0
    for an, (ex, ey), gc in ((dx, (STEP, 0.0), p["gcx"]), (dy, (0.0, STEP), p["gcy"])):
        up, vp, eup, evp = bref.uv64(rl, c["verts"], c["faces"], c["cam"], W, H, X + ex, Y + ey)
        um, vm, eum, evm = bref.uv64(rl, c["verts"], c["faces"], c["cam"], W, H, X - ex, Y - ey)
        q = STEP * gc / p["Dc"]
        keep = live & (np.abs(q) < 0.5)
        assert keep.sum() > 0.99 * live.sum(), (name, int(keep.sum()), int(live.sum()))
        q2 = np.where(keep, q * q, 0.0)
        trunc = q2 / (1.0 - q2)
        fd_u, fd_v = (up - um) / (2 * STEP), (vp - vm) / (2 * STEP)
        ru, rv = 2.0 * (eup + eum) / (2 * STEP), 2.0 * (evp + evm) / (2 * STEP)
        for got, want, tol in ((an[..., 1], fd_u, np.abs(an[..., 1]) * trunc + ru), (an[..., 2], fd_v, np.abs(an[..., 2]) * trunc + rv),
                               (an[..., 0], -(fd_u + fd_v), (np.abs(an[..., 1]) + np.abs(an[..., 2])) * trunc + ru + rv)):
            err = np.abs(got - want)[keep]
            assert (err <= tol[keep]).all(), (name, float((err / tol[keep]).max()))
            worst = max(worst, float((err / np.maximum(np.abs(want[keep]), 1e-30)).max()))
            assert np.abs(want[keep]).max() > 1e-3                              # (the derivatives are there)
    print(name, "worst relative difference to the central differences", worst)


@pytest.mark.parametrize("name,L", [("soup", 3), ("soup", 17), ("lattice", 3)])
def test_float32_order_against_float64(name, L):
    """The float32 restatement within the project's 1e-5 of the tensor's maximum of the same formula in float64."""
    c = case(name, L)
    d32 = bref.forward32(c["layers"], c["verts"], c["faces"], c["cam"], c["W"], c["H"])
    d64 = bref.forward64(c["layers"], c["verts"], c["faces"], c["cam"], c["W"], c["H"])
    for a, b, what in zip(d32, d64, "xy"):
        assert a.dtype == np.float32 and np.isfinite(a).all()
        e = rel_linf(a, b)
        print(name, L, what, "float32 against float64: rel L_inf", e, "max", float(np.abs(b).max()))
        assert e <= 1e-5, (name, L, what, e)


def test_bary_sums_to_zero_and_matches_rasterize():
    """d(bary0) = -(du + dv), and the restatement's (u, v) are rasterize's barycentrics."""
    s = c = case("soup")
    ras = rref.rasterize32(s["W"], s["H"], s["verts"], s["faces"], None, s["verts_ndc"], s["verts_image"], s["ray_o"], s["ray_d"], 3)
    dx, dy, p = bref.forward64(c["layers"], c["verts"], c["faces"], c["cam"], c["W"], c["H"], parts=True)
    assert np.abs(dx.sum(-1)).max() < 1e-12 * np.abs(dx).max()
    hit = c["layers"] >= 0
    assert np.abs(p["u"][hit] - ras["bary"][..., 1][hit]).max() < 1e-3 and np.abs(p["v"][hit] - ras["bary"][..., 2][hit]).max() < 1e-3


def test_empty_and_degenerate_slots_give_zeros():
    c = case("soup")
    F, P = c["faces"].shape[0], c["verts"].shape[0]
    rl = c["layers"][:1, :8, :8].copy()
    rl[0, 0, :4, 0] = [-1, F, F + 7, -2 ** 31]
    faces = c["faces"].copy()
    bad_vertex, flat = 5, 9
    faces[bad_vertex] = [faces[bad_vertex, 0], P, faces[bad_vertex, 2]]
    faces[flat, 2] = faces[flat, 1]                                            # zero area: c = 0, D.c == 0 exactly
    rl[0, 1, 0, 0], rl[0, 1, 1, 0], rl[0, 1, 2, 0] = bad_vertex, flat, 11
    for dt in (np.float32, np.float64):
        dx, dy = bref.forward(rl, c["verts"], faces, c["cam"][:1], c["W"], c["H"], dtype=dt)
        for d in (dx, dy):
            assert not d[0, 0, :4, 0].any() and not d[0, 1, :2, 0].any()
            assert d[0, 1, 2, 0].any() and np.isfinite(d).all()
    z = bref.forward32(rl, c["verts"], faces[:0], c["cam"][:1], c["W"], c["H"])
    assert not z[0].any() and not z[1].any()


def test_window_is_the_crop_of_the_frame():
    c = case("soup")
    full = bref.forward32(c["layers"], c["verts"], c["faces"], c["cam"], c["W"], c["H"])
    pm = np.array([[5, 3], [21, 9], [0, 17]], np.int32)
    ph, pw = 30, 37
    rl = np.stack([c["layers"][b, pm[b, 1]:pm[b, 1] + ph, pm[b, 0]:pm[b, 0] + pw] for b in range(3)])
    win = bref.forward32(rl, c["verts"], c["faces"], c["cam"], c["W"], c["H"], pm)
    for w, f in zip(win, full):
        want = np.stack([f[b, pm[b, 1]:pm[b, 1] + ph, pm[b, 0]:pm[b, 0] + pw] for b in range(3)])
        assert np.array_equal(w.view(np.uint32), want.view(np.uint32))


def test_surface():
    for name in ("BaryDerivativesFunction", "MipmapFunction", "TextureMipFunction"):
        assert name in dm2.__all__ and issubclass(getattr(dm2, name), torch.autograd.Function)
    for name in ("dm2_bary_derivatives_window", "dm2_texture_mipmaps", "dm2_texture_mipmaps_backward", "dm2_texture_mip",
                 "dm2_texture_mip_backward"):
        assert name in _C.EXPORTS
    for cls in (dm2.Renderer, dm2.LayeredRenderer):
        assert callable(cls.bary_derivatives) and callable(cls.texture_mipmaps)
    cpu = torch.zeros((1, 2, 2, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.bary_derivatives_cuda(cpu, torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32), torch.zeros((1, 32)))
