"""Renderer.interpolate without a GPU: the restatement (tests/interpolate_ref.py) against float64 and against float64 torch
autograd of the torch line the op replaces, on hand cases; the interface (C ABI names, module surface, CPU tensors refused)."""
import os
import re

import numpy as np
import pytest
import torch

import interpolate_ref as ref
from util import ROOT

EPS32 = float(np.finfo(np.float32).eps)


def _hand(C, per_view, seed=0):
    """B = 2, 2 x 3 pixels, L = 4, F = 6 faces over N = 7 rows.  Pixel (0,0,0): an empty slot mid-list; (0,0,1): face 2 listed
    twice; face 4 names row 7 (= N) and face 5 row -1: slots listing them are empty; ids -1, 6 (= F), -9 are empty."""
    rng = np.random.RandomState(seed)
    N = 7
    attr_faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3], [1, 7, 2], [-1, 2, 3]], np.int32)
    rl = rng.randint(0, 4, (2, 2, 3, 4)).astype(np.int32)
    rl[0, 0, 0] = [1, -1, 3, 0]
    rl[0, 0, 1] = [2, 0, 2, -1]
    rl[0, 1, 0] = [4, 1, 5, 2]
    rl[1, 0, 2] = [6, -9, 3, 4]
    rl[1, 1, 1] = [-1, -1, -1, -1]
    bary = rng.uniform(-0.2, 1.2, rl.shape + (3,)).astype(np.float32)
    bary[rl < 0] = -1.0
    attr = rng.standard_normal((2, N, C) if per_view else (N, C)).astype(np.float32)
    g = rng.standard_normal(rl.shape + (C,)).astype(np.float32)
    return rl, bary, attr, attr_faces, g


CASES = [(3, False), (1, False), (5, True), (1, True), (16, False)]


@pytest.mark.parametrize("C,per_view", CASES)
def test_forward32_against_float64(C, per_view):
    """|fl32 - exact| <= 2 eps32 sum_k |bary_k| |attr_k|: with u = eps32 / 2, each product carries one rounding and each of the
    two adds one more, so no term is scaled by more than (1 + u)^3 = 1 + 1.5 eps32 + O(eps32^2); float64 stands for exact."""
    rl, bary, attr, af, _ = _hand(C, per_view)
    got = ref.forward32(rl, bary, attr, af)
    want = ref.forward(rl, bary, attr, af, np.float64)
    assert got.dtype == np.float32 and got.shape == rl.shape + (C,)
    assert (np.abs(got.astype(np.float64) - want) <= 2 * EPS32 * ref.forward_bound(rl, bary, attr, af)).all()
    m, _ = ref.filled(rl, af, attr.shape[-2])
    assert m.sum() > 20 and not m[0, 0, 0, 1] and not m[0, 1, 0, 0] and not m[0, 1, 0, 2] and not m[1, 0, 2, 0] and not m[1, 0, 2, 3]
    assert m[0, 0, 0, 2] and m[0, 0, 1, 0] and m[0, 0, 1, 2]
    assert (got[~m] == 0).all() and (np.abs(got[m]).max(-1) > 0).all()


def _torch64(rl, bary, attr, af, g):
    """float64 torch autograd of the one-liner; the slots the contract calls empty are handed over as -1, a row of attr_faces
    outside the table as 0 (no slot reads it then), a per-view table view by view."""
    N = attr.shape[-2]
    m, _ = ref.filled(rl, af, N)
    ids = torch.from_numpy(np.where(m, rl, -1))
    faces = torch.from_numpy(np.where((af >= 0) & (af < N), af, 0))
    b = torch.tensor(bary.astype(np.float64), requires_grad=True)
    a = torch.tensor(attr.astype(np.float64), requires_grad=True)
    if attr.ndim == 3:
        out = torch.stack([ref.one_liner(ids[i:i + 1], b[i:i + 1], a[i], faces)[0] for i in range(attr.shape[0])])
    else:
        out = ref.one_liner(ids, b, a, faces)
    (out * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return out.detach().numpy(), a.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("C,per_view", CASES)
def test_grads64_against_float64_autograd(C, per_view):
    rl, bary, attr, af, g = _hand(C, per_view, seed=1)
    out, dattr_t, dbary_t = _torch64(rl, bary, attr, af, g)
    dattr, dbary = ref.grads64(rl, bary, attr, af, g)
    assert np.abs(out - ref.forward(rl, bary, attr, af, np.float64)).max() <= 1e-14
    assert dattr.shape == attr.shape and dbary.shape == bary.shape
    assert np.abs(dattr).max() > 0 and np.abs(dattr - dattr_t).max() <= 1e-13 * np.abs(dattr_t).max()
    assert np.abs(dbary).max() > 0 and np.abs(dbary - dbary_t).max() <= 1e-13 * np.abs(dbary_t).max()
    m, _ = ref.filled(rl, af, attr.shape[-2])
    assert (dbary[~m] == 0).all()


def test_degenerate_sizes():
    rl, bary, attr, af, g = _hand(3, False)
    z = ref.forward32(rl, bary, attr[:0], af)
    assert z.shape == rl.shape + (3,) and (z == 0).all()
    z = ref.forward32(rl, bary, attr, af[:0])
    assert z.shape == rl.shape + (3,) and (z == 0).all()
    da, db = ref.grads64(rl, bary, attr, af[:0], g)
    assert (da == 0).all() and (db == 0).all()
    assert ref.forward32(rl[..., :0], bary[..., :0, :], attr, af).shape == rl.shape[:3] + (0, 3)


def test_interface():
    """The C ABI declares and exports both entry points, the module has the pair, and CPU tensors are refused."""
    import dmesh2_renderer_amd as dm2
    from dmesh2_renderer_amd import _C, scenes
    header = open(os.path.join(ROOT, "include", "dm2_hip.h")).read()
    for name in ("dm2_interpolate", "dm2_interpolate_backward"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _C.EXPORTS
    assert _C.ABI_VERSION == 8
    assert issubclass(dm2.InterpolateFunction, torch.autograd.Function) and "InterpolateFunction" in dm2.__all__
    assert callable(dm2.Renderer.interpolate) and dm2.LayeredRenderer.interpolate is dm2.Renderer.interpolate
    rl, bary, attr, af, g = (torch.from_numpy(x) for x in _hand(3, False))
    ts = scenes.tet_lattice(32, 24, 2, seed=scenes.SEED_BASE + 3)
    for cls in (dm2.Renderer, dm2.LayeredRenderer):
        r = cls(ts.mv, ts.proj, 32, 24, "cpu", fused_prep=False)
        with pytest.raises(RuntimeError, match="no CPU path"):
            r.interpolate(rl, bary, attr, af)
        with pytest.raises(RuntimeError, match="no CPU path"):
            r.interpolate(rl, bary.clone().requires_grad_(True), attr.clone().requires_grad_(True), af)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.interpolate_backward_cuda(rl, bary, attr, af, g, True, True)
    # the checks name the argument
    with pytest.raises(RuntimeError, match="bary"):
        _C.interpolate_cuda(rl, bary[..., :2], attr, af)
    with pytest.raises(RuntimeError, match="attr_faces"):
        _C.interpolate_cuda(rl, bary, attr, af.reshape(-1))
    with pytest.raises(RuntimeError, match="render_layers"):
        _C.interpolate_cuda(rl[0], bary, attr, af)
    with pytest.raises(RuntimeError, match="attr must"):
        _C.interpolate_cuda(rl, bary, attr[0], af)
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.interpolate_backward_cuda(rl, bary, attr, af, g[..., :2], True, True)
