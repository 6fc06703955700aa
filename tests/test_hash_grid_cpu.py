"""The hash grid contract's restatement (tests/hash_grid_ref.py) held to the integer recurrence and a hash written with Python
integers, to the volume contract's restatement on a single dense level, to a float64 brute force over the levels, its gradients
to central differences, and its edge cases (collisions, the empty rule) to what the contract says of them; and the front end's
and the shim's argument checks, which need no GPU."""
import inspect

import numpy as np
import pytest
import torch

import hash_grid_ref as ref
import texture_volume_ref as vol
from util import assert_own_exports, scenes

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

f32 = np.float32
ISSUE_TABLE = [16, 24, 36, 54, 81, 121, 181, 271, 406, 609, 913, 1369, 2053, 3079, 4618, 6927]


def test_resolutions():
    assert ref.resolutions(16, 16, 24) == ISSUE_TABLE
    assert ref.resolutions(5, 2, 24) == [2, 3, 4, 6, 9]
    assert ref.resolutions(4, 1, 32) == [1, 2, 4, 8]
    assert ref.resolutions(3, 5, 17) == [5, 5, 5]
    assert _C.hash_grid_resolutions(16, 16, 1.5) == ISSUE_TABLE
    assert dm2.Renderer.hash_grid_resolutions(5, 2, 1.5) == [2, 3, 4, 6, 9]
    for NL, N, q in ((7, 3, 17), (9, 11, 29), (32, 1, 20), (1, 77, 32)):
        assert _C.hash_grid_resolutions(NL, N, q / 16) == ref.resolutions(NL, N, q)
        r = ref.resolutions(NL, N, q)
        assert all(b >= a for a, b in zip(r, r[1:]))                       # never decreasing: the finest level decides the range rule
    for growth in (1.0, 1.03, 2.0625, 1.51, 0, -1.5, float("nan")):
        with pytest.raises(ValueError, match="growth"):
            _C.hash_grid_resolutions(4, 16, growth)
    with pytest.raises(ValueError, match="num_levels"):
        _C.hash_grid_resolutions(33, 1, 1.0625)
    with pytest.raises(ValueError, match="num_levels"):
        _C.hash_grid_resolutions(0, 16, 1.5)
    with pytest.raises(ValueError, match="base_resolution"):
        _C.hash_grid_resolutions(4, 0, 1.5)
    assert _C.hash_grid_resolutions(21, 1, 2.0)[-1] == 2 ** 20
    with pytest.raises(ValueError, match="finest"):
        _C.hash_grid_resolutions(22, 1, 2.0)


def test_rows_against_python_integers():
    rng = np.random.default_rng(1)
    for R, T in ((9, 64), (54, 4096), (6927, 2 ** 19), (2 ** 20, 2 ** 24), (1000, 16)):
        assert not ref.is_dense(R, T)
        i, j, k = (rng.integers(0, R, 500) for _ in range(3))
        i[0], j[0], k[0] = R - 1, R - 1, R - 1
        want = [((int(a) ^ (int(b) * 2654435761 % 2 ** 32) ^ (int(c) * 805459861 % 2 ** 32)) % 2 ** 32) % T for a, b, c in zip(i, j, k)]
        got = ref.rows(i, j, k, R, T)
        assert got.dtype == np.int64 and got.tolist() == want
        assert 0 <= got.min() and got.max() < T
    for R, T in ((2, 8), (4, 64), (4, 128), (6, 256), (1, 16), (256, 2 ** 24)):
        assert ref.is_dense(R, T)
        i, j, k = (rng.integers(0, R, 200) for _ in range(3))
        assert ref.rows(i, j, k, R, T).tolist() == [(int(c) * R + int(b)) * R + int(a) for a, b, c in zip(i, j, k)]
    assert not ref.is_dense(5, 124) and ref.is_dense(5, 125)


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("R", (2, 4, 8, 16))
def test_single_dense_level_is_the_volume(R, boundary_mode, filter_mode):
    """T = R^3: the level is the volume contract on table[0].reshape(R, R, R, F), bit for bit forward and in both gradients."""
    rng = np.random.default_rng(R)
    F = 2
    xyz = rng.uniform(-0.6, 1.6, (2, 5, 7, 2, 3)).astype(f32)
    rl = rng.integers(-1, 4, xyz.shape[:4]).astype(np.int32)
    table = rng.standard_normal((1, R ** 3, F)).astype(f32)
    grid = table[0].reshape(R, R, R, F)
    a = ref.forward32(xyz, table, rl, R, 24, filter_mode, boundary_mode)
    b = vol.forward32(xyz, grid, rl, filter_mode, boundary_mode)
    assert a.dtype == f32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    g = rng.standard_normal(a.shape)
    dt, dx = ref.grads64(xyz, table, rl, R, 24, filter_mode, boundary_mode, g)
    dg, dp = vol.grads64(xyz, grid, rl, filter_mode, boundary_mode, g)
    assert np.array_equal(dt.reshape(dg.shape), dg) and np.array_equal(dx, dp)
    at, ax = ref.terms_abs(xyz, table, rl, R, 24, filter_mode, boundary_mode, g)
    ag, ap = vol.terms_abs(xyz, grid, rl, filter_mode, boundary_mode, g)
    assert np.array_equal(at.reshape(ag.shape), ag) and np.array_equal(ax, ap)


def _brute64(xyz, table, N, q, boundary_mode):
    """Trilinear interpolation of every level in float64, slot by slot, with Python integers for the addresses and the hash."""
    NL, T, F = table.shape
    res = ref.resolutions(NL, N, q)
    flat = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros((flat.shape[0], NL, F))
    for s, p in enumerate(flat):
        for l, R in enumerate(res):
            X = p * R - 0.5
            c0 = np.floor(X)
            f = X - c0
            for r in (0, 1):
                for qq in (0, 1):
                    for pp in (0, 1):
                        c = [int(c0[0]) + pp, int(c0[1]) + qq, int(c0[2]) + r]
                        c = [min(max(v, 0), R - 1) if boundary_mode == "clamp" else v % R for v in c]
                        if R ** 3 <= T:
                            row = (c[2] * R + c[1]) * R + c[0]
                        else:
                            row = ((c[0] ^ (c[1] * 2654435761 % 2 ** 32) ^ (c[2] * 805459861 % 2 ** 32)) % 2 ** 32) % T
                        w = (f[0] if pp else 1 - f[0]) * (f[1] if qq else 1 - f[1]) * (f[2] if r else 1 - f[2])
                        out[s, l] += w * table[l, row].astype(np.float64)
    return out.reshape(np.shape(xyz)[:-1] + (NL * F,))


@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("cfg", ((2, 24, 5, 64), (1, 32, 4, 16), (5, 17, 3, 256), (16, 24, 4, 1024)))
def test_forward32_against_a_float64_brute_force(cfg, boundary_mode):
    """1e-5 of the tensor maximum, the project's standing bar; coordinates from -0.4 to 1.4."""
    N, q, NL, T = cfg
    rng = np.random.default_rng(N + NL)
    F = 2
    xyz = rng.uniform(-0.4, 1.4, (1, 5, 8, 2, 3)).astype(f32)
    table = rng.standard_normal((NL, T, F)).astype(f32)
    want = _brute64(xyz, table, N, q, boundary_mode)
    got = ref.forward32(xyz, table, None, N, q, "linear", boundary_mode)
    assert got.shape == want.shape and got.dtype == f32
    err = np.abs(got - want).max() / np.abs(want).max()
    print(cfg, boundary_mode, "forward32 against the brute force", err)
    assert err <= 1e-5
    assert np.abs(ref.forward64(xyz, table, None, N, q, "linear", boundary_mode) - want).max() <= 1e-12 * np.abs(want).max()
    # level-major channels: level l alone is the call's slice l F .. (l + 1) F when the resolutions agree
    res = ref.resolutions(NL, N, q)
    for l in range(NL):
        one = ref.forward32(xyz, np.ascontiguousarray(table[l:l + 1]), None, res[l], q, "linear", boundary_mode)
        assert np.array_equal(one, got[..., l * F:(l + 1) * F])


@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("cfg", ((2, 24, 5, 64), (1, 32, 4, 16), (5, 17, 3, 256)))
def test_grads64_against_central_differences(cfg, boundary_mode):
    """Of forward64, with the float64 stage, away from integer X at every level, where the function has a kink: dL/dxyz by steps of
    the coordinates, dL/dtable (linear in the table) by steps of single elements."""
    N, q, NL, T = cfg
    rng = np.random.default_rng(7 + N)
    F, h = 2, 1e-6
    res = ref.resolutions(NL, N, q)
    xyz = rng.uniform(-0.4, 1.4, (2, 4, 5, 2, 3))
    for _ in range(50):                                                     # move a coordinate off every level's kinks
        near = np.zeros(xyz.shape, bool)
        for R in res:
            X = xyz * R - 0.5
            near |= np.abs(X - np.round(X)) < 0.02
        if not near.any():
            break
        xyz = np.where(near, xyz + 0.013, xyz)
    assert not near.any()
    table = rng.standard_normal((NL, T, F))
    g = rng.standard_normal(xyz.shape[:4] + (NL * F,))
    rl = rng.integers(-1, 4, xyz.shape[:4]).astype(np.int32)
    loss = lambda p, t: (ref.forward64(p, t, rl, N, q, "linear", boundary_mode) * g).sum()
    dtable, dxyz = ref.grads64(xyz, table, rl, N, q, "linear", boundary_mode, g, stage_dtype=np.float64)
    num = np.zeros_like(xyz)
    for a in range(3):
        step = np.zeros_like(xyz)
        step[..., a] = h
        up = (ref.forward64(xyz + step, table, rl, N, q, "linear", boundary_mode) * g).sum(-1)
        dn = (ref.forward64(xyz - step, table, rl, N, q, "linear", boundary_mode) * g).sum(-1)
        num[..., a] = (up - dn) / (2 * h)
    scale = np.abs(num).max()
    assert scale > 0
    assert np.abs(dxyz - num).max() <= 1e-7 * max(scale, 1.0)
    assert not dxyz[rl < 0].any()
    flat = table.reshape(-1)
    touched = np.flatnonzero(dtable.reshape(-1))
    for e in rng.choice(touched, 12, replace=False):
        d = np.zeros_like(flat)
        d[e] = 0.5
        d = d.reshape(table.shape)
        num_e = loss(xyz, table + d) - loss(xyz, table - d)
        assert abs(dtable.reshape(-1)[e] - num_e) <= 1e-9 * max(1.0, abs(num_e))
    dtable32, dxyz32 = ref.grads64(xyz.astype(f32), table, rl, N, q, "linear", boundary_mode, g)
    assert np.abs(dtable32 - dtable).max() <= 1e-5 * np.abs(dtable).max()
    assert np.abs(dxyz32 - dxyz).max() <= 1e-5 * max(np.abs(dxyz).max(), 1.0)
    st, sx = ref.terms_abs(xyz.astype(f32), table, rl, N, q, "linear", boundary_mode, g)
    assert (np.abs(dtable32) <= st * (1 + 1e-12)).all() and (np.abs(dxyz32) <= sx * (1 + 1e-12)).all()
    # nearest: no gradient to the position
    assert not ref.grads64(xyz, table, rl, N, q, "nearest", boundary_mode, g)[1].any()


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_collisions_sum(filter_mode):
    """R = 9, T = 64: 729 voxels on 64 rows.  The level's table gradient is the dense 9^3 grid's gradient (the volume contract's)
    with the voxels of one row summed, and the forward is the dense lookup of the table spread over the voxels."""
    R, T, F = 9, 64, 2
    rng = np.random.default_rng(11)
    xyz = rng.uniform(-0.2, 1.2, (2, 6, 9, 2, 3)).astype(f32)
    table = rng.standard_normal((1, T, F)).astype(f32)
    k, j, i = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    voxel_row = ref.rows(i, j, k, R, T)                                     # (R, R, R)
    assert len(np.unique(voxel_row)) == T and np.bincount(voxel_row.reshape(-1)).max() > 8
    grid = table[0][voxel_row]                                              # (R, R, R, F): every voxel holds its row
    for boundary_mode in ref.BOUNDARIES:
        out = ref.forward32(xyz, table, None, R, 24, filter_mode, boundary_mode)
        assert np.array_equal(out, vol.forward32(xyz, grid, None, filter_mode, boundary_mode))
        g = rng.standard_normal(out.shape)
        dtable, dxyz = ref.grads64(xyz, table, None, R, 24, filter_mode, boundary_mode, g)
        dgrid, dp = vol.grads64(xyz, grid, None, filter_mode, boundary_mode, g)
        summed = np.stack([np.bincount(voxel_row.reshape(-1), weights=dgrid[..., f].reshape(-1), minlength=T) for f in range(F)], -1)
        assert np.abs(dtable[0] - summed).max() <= 1e-12 * np.abs(summed).max()
        assert np.abs(dxyz - dp).max() <= 1e-12 * max(np.abs(dp).max(), 1.0)


def test_empty_rule_at_the_finest_level_is_at_any_level():
    """Negative ids, NaN, infinities and coordinates round the 2^24 bound of the finest level, either side of it, on one axis at
    a time: the rule at the finest level marks the same slots as the rule at any level; empty slots give zeros and get nothing,
    and a NaN table read by nobody stays out of the result."""
    rng = np.random.default_rng(4)
    N, q, NL, T, F, shape = 16, 24, 6, 256, 2, (2, 6, 7, 3)
    res = ref.resolutions(NL, N, q)
    xyz = rng.uniform(0, 1, shape + (3,)).astype(f32)
    rl = rng.integers(0, 5, shape).astype(np.int32)
    bad = rng.uniform(size=shape) < 0.4
    kind = rng.integers(0, 6, shape)
    rl[bad & (kind == 0)] = -1
    edge = 2.0 ** 24 / res[-1]
    for k, val in ((1, np.nan), (2, np.inf), (3, -np.inf), (4, edge + 1.0), (5, -edge)):
        xyz[bad & (kind == k), k % 3] = val
    inside = ~bad & (kind == 4)                                             # just inside the bound: live at the finest level and so at all
    xyz[inside, 1] = f32(edge * 0.999)
    xyz[~bad & (kind == 1), 1] = -0.0
    assert inside.sum() > 5
    e = ref.empty(xyz, res, rl)
    assert np.array_equal(e, bad) and bad.sum() > 60
    assert np.array_equal(e, ref.empty(xyz, res, rl, any_level=True))
    sweep = np.zeros((1, 1, 4000, 1, 3), f32)
    sweep[0, 0, :, 0, 0] = np.concatenate([np.linspace(0.9 * edge, 1.1 * edge, 2000), -np.linspace(0.9 * edge, 1.1 * edge, 2000)])
    es = ref.empty(sweep, res)
    assert es.any() and (~es).any() and np.array_equal(es, ref.empty(sweep, res, any_level=True))
    table = rng.standard_normal((NL, T, F)).astype(f32) + 10
    for filter_mode in ref.FILTERS:
        for boundary_mode in ref.BOUNDARIES:
            out = ref.forward32(xyz, table, rl, N, q, filter_mode, boundary_mode)
            assert (out[bad] == 0).all() and (out[~bad] != 0).all()
            g = rng.standard_normal(out.shape)
            dtable, dxyz = ref.grads64(xyz, table, rl, N, q, filter_mode, boundary_mode, g)
            assert not dxyz[bad].any()
            ones, _ = ref.grads64(xyz, table, rl, N, q, filter_mode, boundary_mode, np.ones(out.shape))
            assert np.allclose(ones.sum(1), (~bad).sum(), rtol=1e-12)       # one unit per live slot and channel into each level
            nobody = np.full_like(table, np.nan)
            assert not ref.forward32(xyz, nobody, np.full(shape, -1, np.int32), N, q, filter_mode, boundary_mode).any()


def test_surface_and_argument_checks():
    assert_own_exports("dm2_hash_grid")                                  # its own two symbols, no value code
    assert "HashGridFunction" in dm2.__all__ and issubclass(dm2.HashGridFunction, torch.autograd.Function)
    assert dm2.LayeredRenderer.hash_grid is dm2.Renderer.hash_grid
    sig = inspect.signature(dm2.Renderer.hash_grid)
    names = ["xyz", "table", "render_layers", "base_resolution", "growth", "filter_mode", "boundary_mode"]
    assert list(sig.parameters) == ["self"] + names
    assert [sig.parameters[k].default for k in names[2:]] == [None, 16, 1.5, "linear", "clamp"]
    for fn in (_C.hash_grid_cuda, _C.hash_grid_backward_cuda):
        assert list(inspect.signature(fn).parameters)[:7] == names
    assert list(inspect.signature(_C.hash_grid_backward_cuda).parameters)[7:] == ["grad_out", "need_table", "need_xyz"]
    assert list(inspect.signature(_C.hash_grid_resolutions).parameters) == ["num_levels", "base_resolution", "growth"]

    p = torch.full((2, 4, 5, 3, 3), 0.5)
    table = torch.zeros((4, 64, 2))
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32)
    for args, name in (((p[..., :2], table, rl), "xyz"), ((p[0], table, rl[0]), "xyz"), ((p, table[0], rl), "table"),
                       ((p, table[:, :48], rl), "table"), ((p, table[:, :8], rl), "table"), ((p, table[:0], rl), "table"),
                       ((p, torch.zeros((4, 64, 3)), rl), "table"), ((p, torch.zeros((33, 16, 1)), rl), "table"),
                       ((p, table, rl[:1]), "render_layers"), ((p, table, rl, 0), "base_resolution"),
                       ((p, table, rl, 16, 1.7), "growth"), ((p, table, rl, 2 ** 20, 2.0), "finest")):
        with pytest.raises(RuntimeError, match=name):
            _C.hash_grid_cuda(*args)
    with pytest.raises(RuntimeError, match="filter_mode"):
        _C.hash_grid_cuda(p, table, rl, 16, 1.5, "cubic")
    with pytest.raises(RuntimeError, match="boundary_mode"):
        _C.hash_grid_cuda(p, table, rl, 16, 1.5, "linear", "cube")
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.hash_grid_backward_cuda(p, table, rl, 16, 1.5, "linear", "clamp", torch.zeros((2, 4, 5, 3, 4)), True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.hash_grid_cuda(p, table, rl)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.hash_grid_backward_cuda(p, table, rl, 16, 1.5, "linear", "wrap", torch.zeros((2, 4, 5, 3, 8)), True, True)

    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None], proj[None], 32, 16, "cpu", fused_prep=False)
    for kw, name in ((dict(filter_mode="linear-mipmap-linear"), "filter_mode"), (dict(boundary_mode="cube"), "boundary_mode"),
                     (dict(growth=1.7), "growth"), (dict(growth=1.0), "growth"), (dict(base_resolution=0), "base_resolution")):
        with pytest.raises(ValueError, match=name):
            r.hash_grid(p, table, rl, **kw)
    for bad_table, name in ((table[:, :48], "T"), (table[:, :8], "T"), (torch.zeros((4, 64, 3)), "F"), (table[0], "table")):
        with pytest.raises(ValueError, match=name):
            r.hash_grid(p, bad_table, rl)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.hash_grid(p, table, rl)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.hash_grid(p.double(), table.double(), rl.long(), 2, 2.0, "nearest", "wrap")     # (the method converts dtypes, as texture3d does)
