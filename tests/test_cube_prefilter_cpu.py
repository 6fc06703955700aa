"""The definition of Renderer.cube_prefilter (tests/cube_prefilter_ref.py, include/dm2_hip.h: dm2_cube_prefilter) on the
CPU: the lobe's symmetry to the bit, self-membership, where the cut bites, the hemisphere at roughness 1, a constant cube, the
first-order cosine convolution against its analytic value; and the shim's and the front end's argument errors, which need no
GPU."""
import inspect

import numpy as np
import pytest
import torch

import cube_prefilter_ref as ref
import texture_cube_ref as cref
from util import assert_own_exports

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

# (n, k, nlev): r = k / (nlev - 1) -> the members per row, smallest and largest
MEMBERS = (((4, 1, 5), (22, 25)), ((8, 1, 6), (30, 46)), ((4, 4, 5), (48, 48)), ((16, 4, 5), (767, 768)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_texels_are_the_lookups_points():
    """d is cref._point over its length, Om = 1 / |p|^3; the solid angles sum to 4 pi up to the centre rule's error."""
    n = 5
    d, om = ref.texels(n)
    for face in range(6):
        for j in range(n):
            for i in range(n):
                p = np.array(cref._point(face, (2 * (i + 0.5)) / n - 1, (2 * (j + 0.5)) / n - 1))
                row = (face * n + j) * n + i
                assert np.allclose(d[row], p / np.linalg.norm(p), rtol=0, atol=3e-7)
                assert np.isclose(om[row], np.linalg.norm(p) ** -3, rtol=5e-7)
    d, om = ref.texels(64)
    assert abs(om.astype(np.float64).sum() * 4 / 64 ** 2 - 4 * np.pi) < 2e-3
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 2e-7


@pytest.mark.parametrize("case,want", MEMBERS)
def test_lobe_symmetry_membership_and_cut(case, want):
    n, k, nlev = case
    r, a2 = ref.roughness(k, nlev)
    K, member = ref.lobe(n, a2)
    assert K.dtype == np.float32 and np.array_equal(_bits(K), _bits(K.T)) and np.array_equal(member, member.T)
    assert member.diagonal().all() and np.array_equal(_bits(K.diagonal()), _bits(np.ones(6 * n * n, np.float32)))
    assert (K[member] > 0).all() and (K[member] <= 1).all() and not K[~member].any()
    per_row = member.sum(1)
    assert (int(per_row.min()), int(per_row.max())) == want
    d, _ = ref.texels(n)
    cos = d.astype(np.float64) @ d.astype(np.float64).T
    if a2 >= 1 / 127:                                                    # the cut never bites: the open hemisphere
        assert np.array_equal(member, cos > 0) or (np.abs(cos[member != (cos > 0)]) < 1e-6).all()
    else:                                                                # every texel left out lies below 1/4096 of the peak
        a2d = float(a2)
        e = a2d + (1 - a2d) * 0.5 * (1 - cos)
        assert ((a2d / e) ** 2 * np.maximum(cos, 0))[~member].max() <= (1 / 4096) * (1 + 1e-5)


def test_cut_is_active_below_r_0_298():
    assert ref.roughness(1, 5)[1] < 1 / 127 < ref.roughness(3, 11)[1]     # r = 0.25, 0.3
    assert abs((1 / 127) ** 0.25 - 0.298) < 5e-4


def test_roughness_one_is_the_cosine_lobe():
    n = 6
    K, member = ref.lobe(n, ref.roughness(3, 4)[1])
    d, _ = ref.texels(n)
    m = ((d[:, None, :].astype(np.float64) - d[None, :, :]) ** 2).sum(-1)
    assert np.abs(K - np.maximum(1 - 0.5 * m, 0)).max() < 1e-6
    assert member.sum() == (K > 0).sum()


def test_constant_cube_stays_constant():
    rng = np.random.default_rng(3)
    for N, mx in ((8, None), (12, None), (16, 2)):
        tex = np.broadcast_to(rng.standard_normal(4).astype(np.float32), (6, N, N, 4)).copy()
        out, tol = ref.prefilter64(tex, mx)
        assert out.shape == (6, ref.layout(N, mx)[2], 4)
        assert np.abs(out - tex[0, 0, 0]).max() <= 1e-12
    assert ref.prefilter64(np.ones((6, 5, 5, 2), np.float32))[0].shape == (6, 0, 2)


def test_first_order_cosine_convolution():
    """n = 16, r = 1: the environment L(l) = l.z comes out as (2/3) n.z, the analytic cosine convolution over pi, within 5e-4
    relative where |n.z| > 1e-3 (what is left is the centre rule's quadrature error)."""
    n, nlev = 16, 5
    A, members = ref.operator(n, nlev - 1, nlev)
    d, _ = ref.texels(n)
    z = d[:, 2].astype(np.float64)
    out = (A @ z) / A.sum(1)
    keep = np.abs(z) > 1e-3
    dev = np.abs(out / ((2.0 / 3.0) * z) - 1)[keep]
    assert keep.sum() == 6 * n * n and dev.max() <= 5e-4, dev.max()


def test_transpose_is_the_adjoint_in_float64():
    rng = np.random.default_rng(5)
    N, C = 8, 2
    T = ref.layout(N)[2]
    x, g = rng.standard_normal((2, 6, T, C)), rng.standard_normal((2, 6, T, C))
    y = ref.primitive64(x, N)[0]
    xb = ref.primitive64(g, N, transpose=True)[0]
    assert abs((y * g).sum() - (x * xb).sum()) <= 1e-12 * np.abs(y * g).sum()
    # and the public op's backward: the derivative of prefilter64, by its linearity
    tex = rng.standard_normal((6, N, N, C)).astype(np.float32)
    gg = rng.standard_normal((6, T, C))
    grad, _ = ref.prefilter_backward64(tex.shape, None, gg)
    out, _ = ref.prefilter64(tex)
    assert abs((out * gg).sum() - (grad * tex).sum()) <= 1e-5 * np.abs(out * gg).sum()     # (the box chain's fp32 roundings)


def test_surface():
    assert "CubePrefilterFunction" in dm2.__all__ and issubclass(dm2.CubePrefilterFunction, torch.autograd.Function)
    assert list(inspect.signature(dm2.Renderer.cube_prefilter).parameters) == ["self", "tex", "max_mip_level", "norm"]
    assert list(inspect.signature(dm2.Renderer.cube_prefilter_norm).parameters) == ["N", "max_mip_level", "device"]
    assert dm2.LayeredRenderer.cube_prefilter is dm2.Renderer.cube_prefilter
    assert_own_exports("dm2_cube_prefilter")                             # its own two symbols, no value code
    for name in ("cube_prefilter_cuda", "cube_prefilter_transpose_cuda"):
        assert callable(getattr(_C, name))


@pytest.mark.parametrize("fn", ("cube_prefilter_cuda", "cube_prefilter_transpose_cuda"))
def test_shim_argument_errors(fn):
    f = getattr(_C, fn)
    T = ref.layout(8)[2]
    with pytest.raises(RuntimeError, match="six faces"):
        f(torch.zeros((5, T, 3)), 8)
    with pytest.raises(RuntimeError, match="six faces"):
        f(torch.zeros((2, 12, T, 3)), 8)
    with pytest.raises(RuntimeError, match="dimensions"):
        f(torch.zeros((T, 3)), 8)
    with pytest.raises(RuntimeError, match="dimensions"):
        f(torch.zeros((6, T + 1, 3)), 8)
    with pytest.raises(RuntimeError, match="dimensions"):
        f(torch.zeros((6, T, 3)), 8, 1)
    with pytest.raises(RuntimeError, match="channel"):
        f(torch.zeros((6, T, 0)), 8)
    with pytest.raises(RuntimeError, match="N must be"):
        f(torch.zeros((6, 0, 3)), 0)
    with pytest.raises(ValueError, match="negative"):
        f(torch.zeros((6, T, 3)), 8, -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(torch.zeros((6, T, 3)), 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(torch.zeros((2, 6, ref.layout(8, 1)[2], 3)), 8, 1)


def test_front_end_argument_errors():
    for shape in ((6, 8, 4, 3), (5, 8, 8, 3), (8, 8, 3), (2, 6, 4, 8, 3)):         # non-square, five faces, no faces
        with pytest.raises(RuntimeError, match="cube_prefilter: tex must have dimensions"):
            dm2.Renderer.cube_prefilter(None, torch.zeros(shape))
    with pytest.raises(RuntimeError, match="norm must have dimensions"):
        dm2.Renderer.cube_prefilter(None, torch.zeros((6, 8, 8, 3)), norm=torch.zeros((6, 5)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dm2.Renderer.cube_prefilter_norm(8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        dm2.Renderer.cube_prefilter(None, torch.zeros((6, 8, 8, 3)), norm=torch.zeros((6, ref.layout(8)[2])))
