"""The numpy restatement of Renderer.texture's contract (tests/texture_ref.py), pinned without the kernels: against torch's
grid_sample on the CPU (linear and nearest, clamp = padding_mode="border", align_corners=False on 2 uv - 1), wrap against
clamp / integer shifts / Python's %, the gradients against float64 central differences and grid_sample's float64 autograd,
and the empty slots.

Measured while writing this test (standard-normal textures, 20 000 samples in [-0.25, 1.25]^2, seed 0), the worst |restatement
- grid_sample| as a share of eps32 x max(Ht, Wt) x (max tex - min tex), float32 / float64 grid_sample:
    1x1 0 / 0, 1x7 0.089 / 0.18, 5x3 0.29 / 0.26, 4x4 0.21 / 0.18, 37x64 0.13 / 0.12, 512x300 0.079 / 0.098,
    300x512 0.074 / 0.10, 2048x2048 0.060 / 3.1e-4
(the test prints them); the bound is 1, so the worst seen is 0.29 of it.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import texture_ref as ref

EPS32 = float(np.finfo(np.float32).eps)
SIZES = ((1, 1), (1, 7), (5, 3), (4, 4), (37, 64), (512, 300), (300, 512), (2048, 2048))       # (Ht, Wt)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _uv(rng, n, lo=-0.25, hi=1.25):
    return rng.uniform(lo, hi, (1, 1, n, 1, 2)).astype(np.float32)


def _grid_sample(tex, uv, mode, dtype):
    """grid_sample on (Ht,Wt,C) tex and (1,1,N,1,2) uv -> (1,1,N,1,C) in ``dtype``."""
    t = torch.from_numpy(np.asarray(tex)).to(dtype).permute(2, 0, 1)[None]
    grid = 2 * torch.from_numpy(np.asarray(uv)).to(dtype).reshape(1, 1, -1, 2) - 1
    out = Fn.grid_sample(t, grid, mode=mode, padding_mode="border", align_corners=False)       # (1,C,1,N)
    return out[0, :, 0].T.reshape(1, 1, -1, 1, tex.shape[-1]).numpy()


@pytest.mark.parametrize("size", SIZES)
def test_linear_clamp_against_grid_sample(size):
    Ht, Wt = size
    rng = np.random.RandomState(0)
    tex = rng.standard_normal((Ht, Wt, 3)).astype(np.float32)
    uv = _uv(rng, 20_000)
    got = ref.forward32(uv, tex, None, "linear", "clamp").astype(np.float64)
    bound = EPS32 * max(Ht, Wt) * float(tex.max() - tex.min())
    for dtype in (torch.float32, torch.float64):
        d = float(np.abs(got - _grid_sample(tex, uv, "bilinear", dtype)).max())
        print(size, dtype, "worst / (eps32 max(Ht, Wt) range) =", d / bound if bound else d)
        assert d <= 1 * bound, (size, dtype, d, bound)


@pytest.mark.parametrize("size", ((5, 3), (64, 64), (37, 64), (300, 512), (2048, 2048)))
def test_nearest_clamp_against_grid_sample(size):
    Ht, Wt = size
    rng = np.random.RandomState(1)
    tex = rng.standard_normal((Ht, Wt, 2)).astype(np.float32)
    uv = _uv(rng, 50_000)
    got = ref.forward32(uv, tex, None, "nearest", "clamp")
    want = _grid_sample(tex, uv, "nearest", torch.float32)
    st = ref.stage(uv, Ht, Wt, None, "nearest", "clamp")
    margin = 4 * EPS32 * max(Ht, Wt)

    def near_integer(x):
        h = x.astype(np.float64) + 0.5
        return np.abs(h - np.round(h)) <= margin
    excused = near_integer(st["x"]) | near_integer(st["y"])
    share = float(excused.mean())
    print(size, "excused share", share)
    assert share < 0.01
    assert np.array_equal(_bits(got[~excused]), _bits(want[~excused]))


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_wrap_equals_clamp_inside(filter_mode):
    rng = np.random.RandomState(2)
    for Ht, Wt in ((4, 4), (37, 64), (512, 300)):
        tex = rng.standard_normal((Ht, Wt, 3)).astype(np.float32)
        m = 1e-3
        u = rng.uniform(0.5 / Wt + m / Wt, 1 - 0.5 / Wt - m / Wt, 10_000)
        v = rng.uniform(0.5 / Ht + m / Ht, 1 - 0.5 / Ht - m / Ht, 10_000)
        uv = np.stack([u, v], -1).astype(np.float32).reshape(1, 1, -1, 1, 2)
        a, b = ref.forward32(uv, tex, None, filter_mode, "wrap"), ref.forward32(uv, tex, None, filter_mode, "clamp")
        assert np.array_equal(_bits(a), _bits(b)), (Ht, Wt)


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_wrap_is_periodic_on_dyadic_uv(filter_mode):
    """Power-of-two sizes and uv = k / 2^10: x is exact in float32, so a shift of uv by an integer gives the same bits."""
    rng = np.random.RandomState(3)
    for Ht, Wt in ((8, 64), (64, 64), (1, 16)):
        tex = rng.standard_normal((Ht, Wt, 3)).astype(np.float32)
        uv = (rng.randint(0, 1024, (1, 1, 5000, 1, 2)) / 1024.0).astype(np.float32)
        base = ref.forward32(uv, tex, None, filter_mode, "wrap")
        for shift in ((1, 0), (0, -1), (-3, 5), (7, -8)):
            moved = (uv + np.array(shift, np.float32)).astype(np.float32)
            assert np.array_equal(moved.astype(np.float64), uv.astype(np.float64) + np.array(shift, np.float64))
            assert np.array_equal(_bits(ref.forward32(moved, tex, None, filter_mode, "wrap")), _bits(base)), (Ht, Wt, shift)
            # a float64 evaluation with Python's %
            u, v = moved[0, 0, :, 0, 0].astype(np.float64), moved[0, 0, :, 0, 1].astype(np.float64)
            x, y = u * Wt - 0.5, v * Ht - 0.5
            t64 = tex.astype(np.float64)
            if filter_mode == "nearest":
                want = np.stack([t64[int(np.floor(yy + 0.5)) % Ht, int(np.floor(xx + 0.5)) % Wt] for xx, yy in zip(x, y)])
            else:
                want = []
                for xx, yy in zip(x, y):
                    i0, j0 = int(np.floor(xx)), int(np.floor(yy))
                    fx, fy = xx - i0, yy - j0
                    t00, t10 = t64[j0 % Ht, i0 % Wt], t64[j0 % Ht, (i0 + 1) % Wt]
                    t01, t11 = t64[(j0 + 1) % Ht, i0 % Wt], t64[(j0 + 1) % Ht, (i0 + 1) % Wt]
                    a, b = t00 + fx * (t10 - t00), t01 + fx * (t11 - t01)
                    want.append(a + fy * (b - a))
                want = np.stack(want)
            assert np.abs(base[0, 0, :, 0] - want).max() <= 4 * EPS32 * np.abs(tex).max()


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
def test_one_texel(filter_mode, boundary_mode):
    tex = np.array([[[1.5, -2.25, 3.0]]], np.float32)
    uv = _uv(np.random.RandomState(4), 1000, -3, 4)
    out = ref.forward32(uv, tex, None, filter_mode, boundary_mode)
    assert np.array_equal(_bits(out), _bits(np.broadcast_to(tex[0, 0], out.shape)))
    # one texel wide, several high: u does not matter
    tex = np.random.RandomState(5).standard_normal((6, 1, 2)).astype(np.float32)
    moved = uv.copy()
    moved[..., 0] = 0.25
    assert np.array_equal(_bits(ref.forward32(uv, tex, None, filter_mode, boundary_mode)),
                          _bits(ref.forward32(moved, tex, None, filter_mode, boundary_mode)))


def _dyadic_uv(rng, shape, Ht, Wt, lo=-0.25, hi=1.25):
    """uv whose x, y are exact in float32 and float64 alike, with fractions in [1/8, 7/8] (Ht, Wt powers of two)."""
    def axis(n):
        cell = rng.randint(int(np.floor(lo * n)) - 1, int(np.ceil(hi * n)) + 1, shape)
        frac = rng.randint(1, 8, shape) / 8.0
        return (cell + frac + 0.5) / n
    return np.stack([axis(Wt), axis(Ht)], -1).astype(np.float32)


@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("per_view", (False, True))
def test_grads64_against_central_differences(boundary_mode, per_view):
    rng = np.random.RandomState(6)
    B, H, W, L, Ht, Wt, C = 2, 3, 4, 2, 4, 8, 2
    uv = _dyadic_uv(rng, (B, H, W, L), Ht, Wt)
    tex = rng.standard_normal((B, Ht, Wt, C) if per_view else (Ht, Wt, C)).astype(np.float32)
    rl = rng.randint(-1, 3, (B, H, W, L)).astype(np.int32)
    g = rng.standard_normal((B, H, W, L, C))
    st32, st64 = (ref.stage(uv, Ht, Wt, rl, "linear", boundary_mode, dt) for dt in (np.float32, np.float64))
    assert np.array_equal(st32["fx"].astype(np.float64), st64["fx"]) and np.array_equal(st32["idx"], st64["idx"])
    dtex, duv = ref.grads64(uv, tex, rl, "linear", boundary_mode, g)

    def loss(uv_, tex_):
        return float((ref.forward(uv_, tex_, rl, "linear", boundary_mode, np.float64) * g).sum())
    t64, uv64 = tex.astype(np.float64), uv.astype(np.float64)
    h = 1e-4
    fd = np.zeros_like(t64)
    for k in range(t64.size):
        p, m = t64.copy(), t64.copy()
        p.reshape(-1)[k] += h
        m.reshape(-1)[k] -= h
        fd.reshape(-1)[k] = (loss(uv64, p) - loss(uv64, m)) / (2 * h)
    assert np.abs(dtex).max() > 0 and np.abs(fd - dtex).max() <= 1e-8 * np.abs(dtex).max()
    h = 1e-3 / max(Ht, Wt)                       # well inside the texel: the fractions are in [1/8, 7/8]
    fd = np.zeros_like(uv64)
    for k in range(uv64.size):
        p, m = uv64.copy(), uv64.copy()
        p.reshape(-1)[k] += h
        m.reshape(-1)[k] -= h
        fd.reshape(-1)[k] = (loss(p, t64) - loss(m, t64)) / (2 * h)
    assert np.abs(duv).max() > 0 and np.abs(fd - duv).max() <= 1e-8 * np.abs(duv).max()
    assert (duv[rl < 0] == 0).all()
    # nearest: weight one on the one texel, nothing to uv
    dtex_n, duv_n = ref.grads64(uv, tex, rl, "nearest", boundary_mode, g)
    assert (duv_n == 0).all()
    fd = np.zeros_like(t64)
    for k in range(t64.size):
        p = t64.copy()
        p.reshape(-1)[k] += 1.0
        fd.reshape(-1)[k] = float(((ref.forward(uv64, p, rl, "nearest", boundary_mode, np.float64)
                                    - ref.forward(uv64, t64, rl, "nearest", boundary_mode, np.float64)) * g).sum())
    assert np.abs(fd - dtex_n).max() <= 1e-12 * max(np.abs(dtex_n).max(), 1.0)


def test_grads64_clamp_against_grid_sample_autograd():
    rng = np.random.RandomState(7)
    Ht, Wt, C, N = 8, 16, 3, 4000
    uv = _dyadic_uv(rng, (1, 1, N, 1), Ht, Wt)
    tex = rng.standard_normal((Ht, Wt, C)).astype(np.float32)
    g = rng.standard_normal((1, 1, N, 1, C))
    dtex, duv = ref.grads64(uv, tex, None, "linear", "clamp", g)
    t = torch.from_numpy(tex).double().requires_grad_(True)
    u = torch.from_numpy(uv).double().requires_grad_(True)
    out = Fn.grid_sample(t.permute(2, 0, 1)[None], (2 * u - 1).reshape(1, 1, N, 2), mode="bilinear", padding_mode="border",
                         align_corners=False)
    (out[0, :, 0].T * torch.from_numpy(g.reshape(N, C))).sum().backward()
    assert np.abs(dtex).max() > 0 and np.abs(duv).max() > 0
    assert np.abs(t.grad.numpy() - dtex).max() <= 1e-12 * np.abs(dtex).max()
    assert np.abs(u.grad.numpy() - duv).max() <= 1e-12 * np.abs(duv).max()
    outside = ((uv < 0) | (uv > 1)).any(-1)
    assert outside.sum() > 500 and (~outside).sum() > 500


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
@pytest.mark.parametrize("per_view", (False, True))
def test_dtex_sums_to_the_upstream_gradient(filter_mode, boundary_mode, per_view):
    """The four weights add to one: dL/dtex sums, per channel, to g summed over the non-empty slots."""
    rng = np.random.RandomState(8)
    B, H, W, L, Ht, Wt, C = 2, 20, 24, 3, 5, 3, 4
    uv = rng.uniform(-2, 3, (B, H, W, L, 2)).astype(np.float32)
    rl = rng.randint(-1, 5, (B, H, W, L)).astype(np.int32)
    tex = rng.standard_normal((B, Ht, Wt, C) if per_view else (Ht, Wt, C)).astype(np.float32)
    g = rng.standard_normal((B, H, W, L, C))
    dtex, _ = ref.grads64(uv, tex, rl, filter_mode, boundary_mode, g)
    live = ~ref.empty(uv, Ht, Wt, rl)
    assert np.array_equal(live, rl >= 0)
    if per_view:
        for b in range(B):
            assert np.allclose(dtex[b].sum((0, 1)), g[b][live[b]].sum(0), rtol=0, atol=1e-9)
    else:
        assert np.allclose(dtex.sum((0, 1)), g[live].sum(0), rtol=0, atol=1e-9)


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
@pytest.mark.parametrize("boundary_mode", ref.BOUNDARIES)
def test_empty_slots(filter_mode, boundary_mode):
    rng = np.random.RandomState(9)
    B, H, W, L, Ht, Wt, C = 1, 8, 8, 2, 4, 4, 2
    uv = rng.uniform(0.4, 0.8, (B, H, W, L, 2)).astype(np.float32)       # x, y in [1.1, 2.7]: no good slot touches texel (0, 0)
    rl = np.zeros((B, H, W, L), np.int32)
    bad = np.zeros((B, H, W, L), bool)
    flat_uv, flat_rl, flat_bad = uv.reshape(-1, 2), rl.reshape(-1), bad.reshape(-1)
    cases = ((np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf), (1e30, 0.5), (0.5, -1e30), (2.0 ** 24, 0.5))
    for k, (u, v) in enumerate(cases):
        flat_uv[3 * k] = (u, v)
        flat_bad[3 * k] = True
    for k in (40, 41, 77):
        flat_rl[k] = -1 - k
        flat_uv[k] = (0.0, 0.0)                                          # what interpolate writes into an empty slot
        flat_bad[k] = True
    assert np.array_equal(ref.empty(uv, Ht, Wt, rl), bad)
    assert np.array_equal(ref.empty(uv, Ht, Wt, None), bad & (rl >= 0))
    tex = rng.standard_normal((Ht, Wt, C)).astype(np.float32) + 10
    out = ref.forward32(uv, tex, rl, filter_mode, boundary_mode)
    assert (out[bad] == 0).all() and (out[~bad] != 0).all()
    g = np.ones((B, H, W, L, C))
    dtex, duv = ref.grads64(uv, tex, rl, filter_mode, boundary_mode, g)
    assert (duv[bad] == 0).all()
    assert (dtex[0, 0] == 0).all() and np.allclose(dtex.sum((0, 1)), (~bad).sum(), rtol=0, atol=1e-9)


def test_distinct_texels_per_tile():
    uv = np.zeros((1, 32, 32, 2, 2), np.float32)
    ys, xs = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    uv[0, :, :, 0, 0], uv[0, :, :, 0, 1] = (xs + 0.5) / 32, (ys + 0.5) / 32      # layer 0: pixel (x, y) on texel (x, y) exactly
    uv[0, :, :, 1] = 0.5 / 32                                                     # layer 1: every pixel on texel (0, 0)
    assert ref.distinct_texels_per_tile(uv, 32, 32, None, "nearest", "clamp") == 1
    assert ref.distinct_texels_per_tile(uv, 32, 32, None, "nearest", "clamp", worst=max) == 256
    assert ref.distinct_texels_per_tile(uv[:, :, :, :1], 32, 32, None, "linear", "clamp") == 256      # (the last tile: i0 + 1 clamps; the first holds 17 x 17)
    rl = np.full((1, 32, 32, 2), -1, np.int32)
    assert ref.distinct_texels_per_tile(uv, 32, 32, rl) == 0


def test_instantiation_inputs_are_what_they_are_for():
    """The inputs of test_gpu_texture.py's test_every_instantiation_once: every tile has live and empty slots in both layers,
    empty by a negative id and by a NaN or infinite uv, and the live uv lie on both sides of both borders."""
    uv, rl = ref.instantiation_case()
    assert uv.shape == ref.INST_SHAPE + (2,) and rl.shape == ref.INST_SHAPE
    e = ref.empty(uv, 5, 3, rl)
    assert ref.tiles_have_live_and_empty(e)
    assert 0.15 < (rl < 0).mean() < 0.35
    bad = ~np.isfinite(uv).all(-1)
    assert bad.sum() == 6 and (rl[bad] >= 0).all() and e[bad].all() and np.isnan(uv).any() and np.isinf(uv).any()
    assert np.array_equal(e, (rl < 0) | bad)
    live = uv[~e]
    assert (live < 0).any(0).all() and (live > 1).any(0).all() and ((live > 0) & (live < 1)).any(0).all()
