"""Group 1 of the mask-driven backward's phase D (dm2_backward_fast.hip) against the form it replaces, as float64 numpy models of
both.  The kernel forms dL/dcolour * intensity once per channel, drops the reference's "0.f +" and folds the clamp's 2 x 2 Jacobian
and i0 = 1 - iuc - ivc into  dL/du = duc_du (dL/di1 - dL/di0) + dvc_du (dL/di2 - dL/di0)  (the same shape for dL/dv), where the
reference (backward.cu:408-488) spells out di_k/du, di_k/dv with their 0 and +-1 factors.  Other orders of the same sums: in
float64 they must agree to rounding, 1e-12 of the largest entry, on all seven clamp codes, and be exactly zero together.

(Group 3 keeps the reference's Jacobian, now from the edge vectors B2 carries: the same operations, nothing to model.  A chain
rule contracted with dL/du, dL/dv first was measured and not kept, profiles/chain_contract_ab.txt.)"""
import numpy as np
import pytest

TOL = 1e-12


def _agree(x, y):
    return np.abs(x - y).max() <= TOL * max(np.abs(x).max(), np.abs(y).max())


def clamp_grad(code):
    """clamp_bary_uv_grad (auxiliary.h:331-357) -> duc_du, duc_dv, dvc_du, dvc_dv"""
    if code == 0:
        return 1.0, 0.0, 0.0, 1.0
    if code in (1, 2, 3):
        return 0.0, 0.0, 0.0, 0.0
    if code == 4:
        return 0.0, 0.0, 0.0, 1.0
    if code == 5:
        return 1.0, 0.0, 0.0, 0.0
    return 0.5, -0.5, -0.5, 0.5


def g1_reference(code, d0, d1, d2):
    """backward.cu:470-480 as the kernel had it: di_k/du, di_k/dv spelled out with their 0 and +-1 factors."""
    duc_du, duc_dv, dvc_du, dvc_dv = clamp_grad(code)
    di0_du, di0_dv = -1.0 * duc_du + -1.0 * dvc_du, -1.0 * duc_dv + -1.0 * dvc_dv
    di1_du, di1_dv = 1.0 * duc_du + 0.0 * dvc_du, 1.0 * duc_dv + 0.0 * dvc_dv
    di2_du, di2_dv = 0.0 * duc_du + 1.0 * dvc_du, 0.0 * duc_dv + 1.0 * dvc_dv
    return (d0 * di0_du + d1 * di1_du + d2 * di2_du, d0 * di0_dv + d1 * di1_dv + d2 * di2_dv)


def g1_folded(code, d0, d1, d2):
    duc_du, duc_dv, dvc_du, dvc_dv = clamp_grad(code)
    d10, d20 = d1 - d0, d2 - d0
    return (duc_du * d10 + dvc_du * d20, duc_dv * d10 + dvc_dv * d20)


def dL_di_reference(i, col, dep, dics, did, intense):
    """dL/di_k and the twelve colour / depth outputs, the reference's operations: three products per term, sums from 0."""
    d = np.zeros(3)
    g = np.zeros(12)
    for ch in range(3):
        for k in range(3):
            d[k] += col[3 * k + ch] * dics[ch] * intense
            g[3 * k + ch] = 0.0 + i[k] * dics[ch] * intense
    for k in range(3):
        d[k] += dep[k] * did
        g[9 + k] = 0.0 + i[k] * did
    return d, g


def dL_di_folded(i, col, dep, dics, did, intense):
    dci = dics * intense
    d = np.array([((col[3 * k] * dci[0] + col[3 * k + 1] * dci[1]) + col[3 * k + 2] * dci[2]) + dep[k] * did for k in range(3)])
    g = np.array([i[k] * dci[ch] for k in range(3) for ch in range(3)] + [i[k] * did for k in range(3)])
    return d, g


@pytest.mark.parametrize("code", range(7))
def test_group1_folded_through_every_clamp_code(code):
    rng = np.random.default_rng(40 + code)
    for _ in range(300):
        i = rng.uniform(0, 1, 3)
        col, dep = rng.uniform(0, 1, 9), rng.uniform(-1, 1, 3)
        dics, did, intense = rng.standard_normal(3), rng.standard_normal(), rng.uniform(0.5, 1.0)
        d_ref, g_ref = dL_di_reference(i, col, dep, dics, did, intense)
        d_new, g_new = dL_di_folded(i, col, dep, dics, did, intense)
        assert _agree(g_ref, g_new) and _agree(d_ref, d_new)
        ref = np.array(g1_reference(code, *d_ref))
        new = np.array(g1_folded(code, *d_new))
        scale = np.abs(d_ref).max()                     # (codes 1..3 give exact zeros on both sides)
        assert np.abs(ref - new).max() <= TOL * scale
        if code in (1, 2, 3):
            assert not ref.any() and not new.any()
