"""The volume contract's restatement (tests/texture_volume_ref.py) held to an independent trilinear (torch's grid_sample in
float64 on the CPU), its gradients to central differences, its edge cases to what the contract says of them; and the front
end's and the shim's argument checks, which need no GPU."""
import inspect

import numpy as np
import pytest
import torch

import texture_volume_ref as ref
from util import assert_own_exports, scenes

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

f32 = np.float32


def _grid(rng, B, N, C, per_view):
    return rng.standard_normal(((B,) if per_view else ()) + (N, N, N, C)).astype(f32)


def _grid_sample64(xyz, grid, boundary_mode, pad=0):
    """torch.nn.functional.grid_sample, float64, align_corners=False: padding_mode="border" for clamp; for wrap the grid padded
    periodically by ``pad`` voxels on every side (the coordinates must stay within it)."""
    B = xyz.shape[0]
    g = np.asarray(grid, np.float64)
    if g.ndim == 4:
        g = np.broadcast_to(g, (B,) + g.shape)
    N = g.shape[1]
    p = np.asarray(xyz, np.float64)
    if boundary_mode == "wrap":
        g = np.pad(g, ((0, 0), (pad, pad), (pad, pad), (pad, pad), (0, 0)), mode="wrap")
        M = N + 2 * pad
        p = (p * N + pad) / M                                             # X' = X + pad in the padded grid
        assert (p * M - 0.5 >= 0).all() and (p * M - 0.5 <= M - 1).all()
    vol = torch.from_numpy(np.ascontiguousarray(g)).permute(0, 4, 1, 2, 3)                  # (B, C, D, H, W)
    H, W, L = p.shape[1:4]
    where = torch.from_numpy(2.0 * p - 1.0).reshape(B, H, W * L, 1, 3).permute(0, 3, 1, 2, 4)      # (B, 1, H, W L, 3)
    out = torch.nn.functional.grid_sample(vol, where, mode="bilinear", padding_mode="border", align_corners=False)
    return out.permute(0, 2, 3, 4, 1).reshape(B, H, W, L, g.shape[-1]).numpy()


@pytest.mark.parametrize("per_view", (False, True))
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("N", (1, 2, 5, 16))
def test_forward32_against_grid_sample(N, boundary_mode, per_view):
    """1e-5 of the tensor maximum, the project's standing bar; coordinates from -0.75 to 1.75, so both modes address beyond
    the grid on every side."""
    rng = np.random.default_rng(1 + N)
    B, C = 2, 3
    xyz = rng.uniform(-0.75, 1.75, (B, 9, 11, 2, 3)).astype(f32)
    grid = _grid(rng, B, N, C, per_view)
    want = _grid_sample64(xyz, grid, boundary_mode, pad=N + 1)
    got = ref.forward32(xyz, grid, None, "linear", boundary_mode)
    assert got.dtype == f32 and got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    print(N, boundary_mode, per_view, "forward32 against grid_sample", err)
    assert err <= 1e-5
    assert np.abs(ref.forward64(xyz, grid, None, "linear", boundary_mode) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("N", (1, 3))
def test_voxel_centres_and_nearest(N, boundary_mode):
    """At a voxel centre exactly every fraction is 0 and both filters return the voxel to the bit; nearest agrees with linear's
    heaviest tap elsewhere."""
    rng = np.random.default_rng(2)
    grid = _grid(rng, 1, N, 2, False)
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    xyz = (np.stack([i, j, k], -1).reshape(1, 1, -1, 1, 3) + 0.5) / N
    assert np.array_equal((xyz.astype(f32) * f32(N) - f32(0.5)), np.stack([i, j, k], -1).reshape(1, 1, -1, 1, 3))
    for filter_mode in ref.FILTERS:
        out = ref.forward32(xyz, grid, None, filter_mode, boundary_mode)
        assert np.array_equal(out.reshape(N, N, N, 2), grid), filter_mode
    p = rng.uniform(-0.5, 1.5, (1, 4, 50, 2, 3)).astype(f32)
    st = ref.stage(p, N, None, "linear", boundary_mode)
    f = st["f"].astype(np.float64)
    tap = ((f[..., 0] >= 0.5) * 1 + (f[..., 1] >= 0.5) * 2 + (f[..., 2] >= 0.5) * 4)
    heavy = np.take_along_axis(st["idx"], tap[..., None], -1)[..., 0]
    near = ref.stage(p, N, None, "nearest", boundary_mode)["idx"][..., 0]
    clear = (np.abs(f - 0.5) > 1e-3).all(-1)                                # (floor(X + 0.5) rounds where f is 0.5 to the last bit)
    assert clear.sum() > 300 and np.array_equal(heavy[clear], near[clear])


def test_the_unit_cubes_faces_and_beyond():
    """x = 0 is half a voxel before the first centre: X = -0.5, i0 = -1, fx = 0.5.  clamp folds both taps onto voxel 0 (the
    voxel itself, to the bit); wrap blends voxel N - 1 and voxel 0 in equal parts.  x = 1 alike at the other end.  Beyond
    [0, 1] clamp stays constant, and wrap has period 1 wherever the shift by N is exact in float32."""
    N, C = 4, 1
    grid = np.arange(N * N * N * C, dtype=f32).reshape(N, N, N, C)
    c = (1 + 0.5) / N                                                        # centre of voxel 1 on the other two axes
    for axis in range(3):
        stride = N ** axis                                                   # x: the last spatial axis
        at = lambda v: np.array([v if a == axis else c for a in range(3)], f32).reshape(1, 1, 1, 1, 3)
        v0 = float(grid.reshape(-1)[1 * (1 + N + N * N) - stride])           # voxel 0 along ``axis``, 1 on the others
        vl = v0 + (N - 1) * stride
        for x, want_clamp in ((0.0, v0), (-0.0, v0), (1.0, vl), (-3.25, v0), (7.5, vl)):
            assert ref.forward32(at(x), grid, None, "linear", "clamp")[0, 0, 0, 0, 0] == want_clamp, (axis, x)
        for x in (0.0, -0.0, 1.0, 3.0, -2.0):
            assert ref.forward32(at(x), grid, None, "linear", "wrap")[0, 0, 0, 0, 0] == 0.5 * (v0 + vl), (axis, x)
        st = ref.stage(at(0.0), N, None, "linear", "wrap")
        assert st["f"][0, 0, 0, 0, axis] == 0.5 and st["X"][0, 0, 0, 0, axis] == -0.5
        for x in (0.3125, 0.875):                                            # multiples of 1 / 16: x + m exact
            a = ref.forward32(at(x), grid, None, "linear", "wrap")
            for m in (-2.0, 1.0, 5.0):
                assert np.array_equal(a, ref.forward32(at(x + m), grid, None, "linear", "wrap")), (axis, x, m)


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
def test_one_voxel_grid(filter_mode, boundary_mode):
    """N = 1: all eight taps are the one voxel; the output is it to the bit, its gradient collects every slot's g, and the
    position's gradient is zero."""
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-2, 3, (1, 5, 6, 2, 3)).astype(f32)
    grid = _grid(rng, 1, 1, 3, False)
    out = ref.forward32(xyz, grid, None, filter_mode, boundary_mode)
    assert np.array_equal(out, np.broadcast_to(grid.reshape(3), out.shape))
    g = rng.standard_normal(out.shape)
    dgrid, dxyz = ref.grads64(xyz, grid, None, filter_mode, boundary_mode, g)
    assert np.allclose(dgrid.reshape(3), g.sum((0, 1, 2, 3)), rtol=1e-12)
    assert np.abs(dxyz).max() <= 1e-14 * np.abs(g).max() * np.abs(grid).max()       # (the float64 sum of dw_k t cancels to rounding)


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
def test_empty_slots(filter_mode, boundary_mode):
    """Negative ids, NaN, infinities and coordinates beyond the 2^24 range rule on any one axis: zeros out, no gradient, and
    a NaN grid read by nobody else stays out of the result.  -0.0 is a coordinate like any other."""
    rng = np.random.default_rng(4)
    N, C, shape = 4, 2, (2, 6, 7, 3)
    xyz = rng.uniform(0, 1, shape + (3,)).astype(f32)
    rl = rng.integers(0, 5, shape).astype(np.int32)
    bad = rng.uniform(size=shape) < 0.4
    kind = rng.integers(0, 6, shape)
    rl[bad & (kind == 0)] = -1
    for k, val in ((1, np.nan), (2, np.inf), (3, -np.inf), (4, 2.0 ** 24 / N + 1.0), (5, -(2.0 ** 24) / N)):
        xyz[bad & (kind == k), k % 3] = val
    xyz[~bad & (kind == 1), 1] = -0.0
    assert np.array_equal(ref.empty(xyz, N, rl), bad) and bad.sum() > 60
    grid = _grid(rng, 2, N, C, True) + 10
    out = ref.forward32(xyz, grid, rl, filter_mode, boundary_mode)
    assert (out[bad] == 0).all() and (out[~bad] != 0).all()
    g = rng.standard_normal(shape + (C,))
    dgrid, dxyz = ref.grads64(xyz, grid, rl, filter_mode, boundary_mode, g)
    assert not dxyz[bad].any()
    ones, _ = ref.grads64(xyz, grid, rl, filter_mode, boundary_mode, np.ones(shape + (C,)))
    assert np.allclose(ones.sum((0, 1, 2, 3)), (~bad).sum(), rtol=1e-12)   # one unit of weight per live slot and channel
    # view 1's grid all NaN and every slot of view 1 empty: nothing of it arrives anywhere
    grid[1] = np.nan
    rl[1] = -1
    out = ref.forward32(xyz, grid, rl, filter_mode, boundary_mode)
    assert np.isfinite(out).all() and not out[1].any()
    assert all(np.isfinite(x).all() for x in ref.grads64(xyz, grid, rl, filter_mode, boundary_mode, g))


@pytest.mark.parametrize("per_view", (False, True))
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("N", (1, 2, 5))
def test_grads64_against_central_differences(N, boundary_mode, per_view):
    """Of forward64, with the float64 stage (the derivative the float32 stage's differs from by its fractions' rounding), away
    from integer X, where the function has a kink: dL/dxyz by steps of the coordinates, dL/dgrid (linear in the grid) by steps
    of single voxels."""
    rng = np.random.default_rng(5 + N)
    B, C, h = 2, 2, 1e-6
    xyz = rng.uniform(-0.6, 1.6, (B, 4, 5, 2, 3))
    X = xyz * N - 0.5
    xyz = np.where(np.abs(X - np.round(X)) < 0.05, xyz + 0.1 / N, xyz)
    grid = _grid(rng, B, N, C, per_view).astype(np.float64)
    g = rng.standard_normal(xyz.shape[:4] + (C,))
    rl = rng.integers(-1, 4, xyz.shape[:4]).astype(np.int32)
    loss = lambda p, q: (ref.forward64(p, q, rl, "linear", boundary_mode) * g).sum()
    dgrid, dxyz = ref.grads64(xyz, grid, rl, "linear", boundary_mode, g, stage_dtype=np.float64)
    num = np.zeros_like(xyz)
    for a in range(3):
        step = np.zeros_like(xyz)
        step[..., a] = h
        up = (ref.forward64(xyz + step, grid, rl, "linear", boundary_mode) * g).sum(-1)
        dn = (ref.forward64(xyz - step, grid, rl, "linear", boundary_mode) * g).sum(-1)
        num[..., a] = (up - dn) / (2 * h)
    scale = np.abs(num).max()
    if N > 1:
        assert scale > 0
    assert np.abs(dxyz - num).max() <= 1e-7 * max(scale, 1.0)
    assert not dxyz[rl < 0].any()
    flat = grid.reshape(-1)
    for e in rng.choice(flat.size, min(flat.size, 12), replace=False):
        d = np.zeros_like(flat)
        d[e] = 0.5
        d = d.reshape(grid.shape)
        num_e = loss(xyz, grid + d) - loss(xyz, grid - d)
        assert abs(dgrid.reshape(-1)[e] - num_e) <= 1e-9 * max(1.0, abs(num_e))
    # the float32 stage moves the fractions by a few ulps of X: the two derivatives agree to float32's precision
    dgrid32, dxyz32 = ref.grads64(xyz.astype(f32), grid, rl, "linear", boundary_mode, g)
    assert np.abs(dgrid32 - dgrid).max() <= 1e-5 * max(np.abs(dgrid).max(), 1e-30)
    assert np.abs(dxyz32 - dxyz).max() <= 1e-5 * max(np.abs(dxyz).max(), 1.0)
    # every term by its absolute value bounds the sums
    sg, sx = ref.terms_abs(xyz.astype(f32), grid, rl, "linear", boundary_mode, g)
    assert (np.abs(dgrid32) <= sg * (1 + 1e-12)).all() and (np.abs(dxyz32) <= sx * (1 + 1e-12)).all()


def test_distinct_voxels_per_tile():
    rng = np.random.default_rng(8)
    xyz = rng.uniform(0, 1, (1, 32, 32, 2, 3)).astype(f32)
    assert ref.distinct_voxels_per_tile(xyz, 32) > 1000                      # unrelated positions: about 8 voxels per slot
    flat = np.full((1, 32, 32, 2, 3), 0.5, f32)                              # every slot in one cell
    assert ref.distinct_voxels_per_tile(flat, 32, worst=max) == 8
    assert ref.distinct_voxels_per_tile(flat, 32, filter_mode="nearest", worst=max) == 1
    assert ref.distinct_voxels_per_tile(flat, 32, np.full((1, 32, 32, 2), -1, np.int32), worst=max) == 0


def test_surface_and_argument_checks():
    assert_own_exports("dm2_texture_volume")                             # its own two symbols, no value code
    assert set(ref.BOUNDARIES) == set(_C.TEX_BOUNDARIES) and _C._TEXTURE_VOLUME.boundaries is _C.TEX_BOUNDARIES
    lib = _C.load_library()                                              # ABI 7's words, still named in the shim: refused (no GPU needed)
    for word in _C.TEX_VOLUME_BOUNDARIES.values():
        for filt in _C.TEX_FILTERS.values():
            assert lib.dm2_texture_cube(2, 4, 5, 3, 8, 3, 0, filt | word, *[None] * 5) == 1
            assert b"unknown filter" in lib.dm2_last_error()
            assert lib.dm2_texture_cube_backward(2, 4, 5, 3, 8, 3, 0, filt | word, *[None] * 7) == 1
    assert "TextureVolumeFunction" in dm2.__all__ and issubclass(dm2.TextureVolumeFunction, torch.autograd.Function)
    assert dm2.LayeredRenderer.texture3d is dm2.Renderer.texture3d
    sig = inspect.signature(dm2.Renderer.texture3d)
    assert list(sig.parameters) == ["self", "xyz", "grid", "render_layers", "filter_mode", "boundary_mode"]
    assert [sig.parameters[k].default for k in ("render_layers", "filter_mode", "boundary_mode")] == [None, "linear", "clamp"]
    for fn in (_C.texture_volume_cuda, _C.texture_volume_backward_cuda):
        assert list(inspect.signature(fn).parameters)[:5] == ["xyz", "grid", "render_layers", "filter_mode", "boundary_mode"]
    assert list(inspect.signature(_C.texture_volume_backward_cuda).parameters)[5:] == ["grad_out", "need_grid", "need_xyz"]

    p = torch.full((2, 4, 5, 3, 3), 0.5)
    grid = torch.zeros((8, 8, 8, 3))
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32)
    for args, name in (((p[..., :2], grid, rl), "xyz"), ((p[0], grid, rl[0]), "xyz"),
                       ((p, grid[0], rl), "grid"), ((p, grid[None].expand(3, 8, 8, 8, 3), rl), "grid"), ((p, grid[:7], rl), "grid"),
                       ((p, grid[:, :7], rl), "grid"), ((p, grid[:, :, :7], rl), "grid"), ((p, grid[:0, :0, :0], rl), "grid"),
                       ((p, grid[..., :0], rl), "grid"), ((p, grid, rl[:1]), "render_layers")):      # (dtypes: checked past the device, on the GPU)
        with pytest.raises(RuntimeError, match=name):
            _C.texture_volume_cuda(*args)
    with pytest.raises(RuntimeError, match="filter_mode"):
        _C.texture_volume_cuda(p, grid, rl, "cubic")
    with pytest.raises(RuntimeError, match="boundary_mode"):
        _C.texture_volume_cuda(p, grid, rl, "linear", "cube")
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.texture_volume_backward_cuda(p, grid, rl, "linear", "clamp", torch.zeros((2, 4, 5, 3, 2)), True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_volume_cuda(p, grid, rl)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_volume_backward_cuda(p, grid, rl, "linear", "wrap", torch.zeros((2, 4, 5, 3, 3)), True, True)

    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None], proj[None], 32, 16, "cpu", fused_prep=False)
    with pytest.raises(ValueError, match="filter_mode"):
        r.texture3d(p, grid, rl, filter_mode="linear-mipmap-linear")
    with pytest.raises(ValueError, match="boundary_mode"):
        r.texture3d(p, grid, rl, boundary_mode="cube")
    with pytest.raises(RuntimeError, match="grid"):
        r.texture3d(p, grid[:7], rl)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.texture3d(p, grid, rl)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.texture3d(p.double(), grid.double(), rl.long(), "nearest", "wrap")       # (the method converts dtypes, as texture does)
