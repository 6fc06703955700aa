"""The restatement of Renderer.shading_vectors (tests/shading_ref.py), without a GPU: the geometry of the reflection, its bits
under n -> -n, the orthogonality of the normal's gradient, grads64 against float64 central differences, and the empty-slot
rules."""
import numpy as np
import pytest
import torch

import shading_ref as sref

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

f32 = np.float32
EPS32 = float(np.finfo(f32).eps)


def _case(seed=0, B=2, H=3, W=5, L=3):
    rng = np.random.default_rng(seed)
    layers = rng.integers(-1, 6, (B, H, W, L)).astype(np.int32)
    t = rng.uniform(0.5, 4.0, (B, H, W, L)).astype(f32)
    t[layers < 0] = -1.0                                                   # as rasterize leaves an empty slot
    n = (rng.standard_normal((B, H, W, L, 3)) * rng.uniform(0.1, 5.0, (B, H, W, L, 1))).astype(f32)
    ro = np.broadcast_to(rng.uniform(-1, 1, (B, 1, 1, 3)), (B, H, W, 3)).astype(f32)
    rd = rng.standard_normal((B, H, W, 3))
    rd = (rd / np.linalg.norm(rd, axis=-1, keepdims=True)).astype(f32)
    return layers, t, n, ro, rd


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_reflection_geometry():
    layers, t, n, ro, rd = _case()
    pos, view, nrm, refl = (x.astype(np.float64) for x in sref.forward32(layers, t, n, ro, rd))
    live = layers >= 0
    assert live.any() and (~live).any()
    assert np.abs(np.linalg.norm(refl[live], axis=-1) - 1).max() <= 8 * EPS32
    assert np.abs(np.linalg.norm(nrm[live], axis=-1) - 1).max() <= 4 * EPS32
    assert np.abs((refl * nrm).sum(-1) - (view * nrm).sum(-1))[live].max() <= 8 * EPS32
    want = ro[:, :, :, None, :].astype(np.float64) + t[..., None].astype(np.float64) * rd[:, :, :, None, :]
    assert np.abs(pos - want)[live].max() <= 4 * EPS32 * np.abs(want).max()
    assert np.array_equal(_bits(view.astype(f32))[live], _bits(np.broadcast_to(-rd[:, :, :, None, :], view.shape).astype(f32))[live])
    two = sref.forward32(layers, t, None, ro, rd)
    assert len(two) == 2 and np.array_equal(_bits(two[0]), _bits(pos.astype(f32))) and np.array_equal(_bits(two[1]), _bits(view.astype(f32)))


def test_reflection_does_not_see_the_sign_of_the_normal():
    layers, t, n, ro, rd = _case(1)
    a = sref.forward32(layers, t, n, ro, rd)
    b = sref.forward32(layers, t, -n, ro, rd)
    assert np.array_equal(_bits(a[3]), _bits(b[3])) and a[3].any()
    live = layers >= 0
    assert np.array_equal(a[2][live], -b[2][live])


def test_empty_slot_rules():
    layers, t, n, ro, rd = _case(2, B=1, H=2, W=4, L=2)
    layers[:] = 3
    layers[0, 0, 0, 0] = -1
    t[0, 0, 1, 0], t[0, 0, 1, 1], t[0, 0, 2, 0] = np.nan, np.inf, -np.inf
    t[0, 0, 2, 1] = -0.0                                                   # finite: not empty
    n[0, 1, 0, 0] = (-0.0, 0.0, -0.0)                                      # zero length
    n[0, 1, 0, 1] = (np.nan, 1.0, 0.0)
    n[0, 1, 1, 0] = (1.0, np.inf, 0.0)
    n[0, 1, 1, 1] = (3e38, 3e38, 0.0)                                      # finite components, nl overflows
    pos, view, nrm, refl = sref.forward32(layers, t, n, ro, rd)
    for s in ((0, 0, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1), (0, 0, 2, 0)):
        for out in (pos, view, nrm, refl):
            assert np.array_equal(_bits(out[s]), np.zeros(3, np.uint32)), s          # +0.0, not -0.0
    assert np.array_equal(pos[0, 0, 2, 1], ro[0, 0, 2] + f32(-0.0) * rd[0, 0, 2]) and nrm[0, 0, 2, 1].any()
    for s in ((0, 1, 0, 0), (0, 1, 0, 1), (0, 1, 1, 0), (0, 1, 1, 1)):
        assert np.array_equal(_bits(nrm[s]), np.zeros(3, np.uint32)) and np.array_equal(_bits(refl[s]), np.zeros(3, np.uint32)), s
        assert view[s].any() and np.isfinite(pos[s]).all()
    assert np.isfinite(np.concatenate([x.reshape(-1) for x in (pos, view, nrm, refl)])).all()
    g = np.random.default_rng(0).standard_normal(pos.shape)
    dt, dn, st, sn = sref.grads64(layers, t, n, ro, rd, g, g, g)
    for s in ((0, 0, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1), (0, 0, 2, 0)):
        assert dt[s] == 0 and not dn[s].any() and st[s] == 0 and not sn[s].any()
    for s in ((0, 1, 0, 0), (0, 1, 0, 1), (0, 1, 1, 0), (0, 1, 1, 1)):
        assert dt[s] != 0 and not dn[s].any() and not sn[s].any()
    assert np.isfinite(dt).all() and np.isfinite(dn).all()


@pytest.mark.parametrize("which", ["all", "position", "normal", "reflection"])
def test_grads64_against_central_differences(which):
    layers, t, n, ro, rd = _case(3, B=1, H=2, W=3, L=2)
    rng = np.random.default_rng(7)
    gs = [rng.standard_normal(n.shape) if which in ("all", k) else None for k in ("position", "normal", "reflection")]
    dt, dn, st, sn = sref.grads64(layers, t, n, ro, rd, *gs)
    live = layers >= 0
    h = 1e-6
    t64, n64 = np.where(live, t, 0.0).astype(np.float64), n.astype(np.float64)
    wt, wn = np.zeros_like(t64), np.zeros_like(n64)
    for arr, out, key in ((t64, wt, "t64"), (n64, wn, "n64")):
        for idx in np.ndindex(*arr.shape):
            keep = arr[idx]
            arr[idx] = keep + h
            hi = sref.loss64(layers, t, n, ro, rd, *gs, t64=t64, n64=n64)
            arr[idx] = keep - h
            lo = sref.loss64(layers, t, n, ro, rd, *gs, t64=t64, n64=n64)
            arr[idx] = keep
            out[idx] = (hi - lo) / (2 * h)
    scale = max(np.abs(wt).max(), np.abs(wn).max())
    assert scale > 0
    assert np.abs(dt - wt).max() <= 1e-6 * scale and np.abs(dn - wn).max() <= 1e-6 * scale
    assert (np.abs(dt) <= st * (1 + 1e-12)).all() and (np.abs(dn) <= sn * (1 + 1e-12)).all()
    assert not dt[~live].any() and not dn[~live].any()
    # the normal's gradient is orthogonal to the normal; position alone sends it nothing
    assert np.abs((dn * n64).sum(-1)).max() <= 1e-12 * max(np.abs(dn).max(), 1.0) * np.abs(n64).max()
    if which == "position":
        assert not dn.any() and dt[live].all()
    if which in ("normal", "reflection"):
        assert not dt.any() and dn[live].any()


def test_surface():
    for name in ("dm2_shading_vectors_window", "dm2_shading_vectors_backward_window"):
        assert name in _C.EXPORTS
    rl = torch.zeros((1, 2, 2, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.shading_vectors_cuda(rl, torch.zeros((1, 2, 2, 1)), None, torch.zeros((1, 2, 2, 3)), torch.zeros((1, 2, 2, 3)))
    from dmesh2_renderer_amd import scenes
    mv, proj = scenes.camera(2, 2)
    r = dm2.Renderer(mv[None], proj[None], 2, 2, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.shading_vectors([0], rl, torch.zeros((1, 2, 2, 1)))
    with pytest.raises(ValueError, match="render_layers"):
        r.shading_vectors([0], rl[0], torch.zeros((2, 2, 1)))
    with pytest.raises(ValueError, match="patch_min"):
        r.shading_vectors([0], torch.zeros((1, 3, 2, 1), dtype=torch.int32), torch.zeros((1, 3, 2, 1)))
