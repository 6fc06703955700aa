"""The restatement of the mip chain and of trilinear sampling (tests/texture_mip_ref.py), without a GPU: the level of detail
against the exact logarithm, level 0 against texture_ref, the chain's layout and adjoint, grads64 against finite differences,
what the inputs of the GPU tests reach, what the feature is for (a minified checkerboard), and a twin for every further input
set of tests/test_gpu_texture_mip.py: the condition that GPU test relies on, asserted with numpy alone."""
import numpy as np
import pytest

import texture_mip_ref as mref
import texture_ref as tref

from dmesh2_renderer_amd import _C

f32 = np.float32
SHAPE = (2, 20, 24, 3)
TEXTURES = ((16, 8), (8, 8), (6, 10), (5, 7))            # (Ht, Wt): nlev 4, 4, 2, 1


def test_layout():
    for (Ht, Wt, mx), (nlev, T) in {(2048, 2048, None): (12, (4 ** 11 - 1) // 3), (16, 8, None): (4, 32 + 8 + 2), (6, 10, None): (2, 15),
                                    (5, 7, None): (1, 0), (16, 8, 1): (2, 32), (16, 8, 0): (1, 0)}.items():
        n, levels, t = mref.layout(Ht, Wt, mx)
        assert (n, t) == (nlev, T), (Ht, Wt, mx, n, t)
        assert (n, levels, t) == _C.mip_layout(Ht, Wt, mx)
        off = 0
        for k in range(1, n):
            assert levels[k] == (Ht >> k, Wt >> k, off)
            off += levels[k][0] * levels[k][1]
    assert mref.layout(16, 8)[1][-1][:2] == (2, 1)
    with pytest.raises(ValueError):
        _C.mip_layout(8, 8, -1)


def test_lod_against_the_exact_logarithm():
    """lod = 0.5 (e + (m - 1)) never exceeds 0.5 log2(r2) and falls short of it by at most 0.04304 levels: e + (m - 1) and
    m - 1 are exact in float32, the sum and the halving round once, so lod carries at most half an ulp of itself."""
    rng = np.random.RandomState(3)
    s = (2.0 ** rng.uniform(0.0, 20.0, 200_000)).astype(f32)
    da = np.stack([s, np.zeros_like(s), np.zeros_like(s), np.zeros_like(s)], -1)
    lod, r2 = mref.lod32(da, 1, 1)
    keep = r2 > 1
    exact = 0.5 * np.log2(r2[keep].astype(np.float64))
    err = exact - lod[keep].astype(np.float64)
    print("lod shortfall: min", err.min(), "max", err.max())
    assert (err >= -lod[keep] * 2.0 ** -24).all() and err.max() <= 0.0431
    assert err.max() > 0.0429 and abs(mref.LOD_SHORTFALL - 0.04304) < 1e-5     # (the bound is reached)
    # the other axis, the larger of the two, and r2 <= 1
    assert mref.lod32(np.array([[0.1, 0.2, 3.0, 4.0]], f32), 1, 1)[0][0] == f32(0.5) * (f32(4) + (f32(25.0 / 16) - f32(1)))
    assert mref.lod32(np.array([[0.5, 0.5, 0.25, 0.1]], f32), 1, 1)[0][0] == 0 and mref.lod32(np.array([[1, 0, 0, 0]], f32), 1, 1)[0][0] == 0
    assert mref.lod32(np.array([[1e30, 0, 0, 0]], f32), 1, 1)[0][0] == 64.0    # r2 = infinity: e = 128, m = 1


@pytest.mark.parametrize("size", TEXTURES)
def test_inputs_reach_every_branch(size):
    uv, da, rl = mref.case(SHAPE, *size, seed=11)
    r = mref.reach(uv, da, *size, rl)
    print(size, r)
    nlev = mref.layout(*size)[0]
    assert r["magnified"] > 0 and r["empty_id"] > 0 and r["empty_uv"] > 0 and r["empty_da"] > 0
    assert len(r["pairs"]) == nlev - 1 and all(n > 0 for n in r["pairs"])
    assert r["beyond"] > 0                                                  # (one level: every minified slot)
    r1 = mref.reach(uv, da, 16, 8, rl, max_mip_level=1)
    assert len(r1["pairs"]) == 1 and r1["pairs"][0] > 0 and r1["beyond"] > 0


@pytest.mark.parametrize("boundary_mode", mref.BOUNDARIES)
def test_level_zero_is_the_linear_filter(boundary_mode):
    """Where lod <= 0 the result is texture_ref.forward32(..., "linear")'s, to the bit."""
    rng = np.random.default_rng(5)
    for size in TEXTURES:
        uv, da, rl = mref.case(SHAPE, *size, seed=12)
        tex = rng.standard_normal(size + (3,), dtype=f32)
        mip = mref.mipmaps(tex)
        st = mref.stage(uv, da, *size, rl)
        low = ~st["empty"] & (st["lod"] <= 0)
        assert low.sum() > 50
        got = mref.forward32(uv, da, tex, mip, rl, boundary_mode)
        want = tref.forward32(uv, tex, rl, "linear", boundary_mode)
        assert np.array_equal(got[low].view(np.uint32), want[low].view(np.uint32))
        assert not got[st["empty"]].any()
        two = st["two"]
        if two.any():
            assert (got[two] != want[two]).any()


def test_constant_texture_gives_the_constant_at_every_lod():
    for size in TEXTURES:
        uv, da, rl = mref.case(SHAPE, *size, seed=13)
        tex = np.full((2,) + size + (2,), f32(0.7))
        tex[1] = f32(-3.25)
        mip = mref.mipmaps(tex)
        assert mip.shape == (2, mref.layout(*size)[2], 2) and (mip[0] == f32(0.7)).all() and (mip[1] == f32(-3.25)).all()
        out = mref.forward32(uv, da, tex, mip, rl, "wrap")
        live = ~mref.stage(uv, da, *size, rl)["empty"]
        assert (out[0][live[0]] == f32(0.7)).all() and (out[1][live[1]] == f32(-3.25)).all() and not out[~live].any()


def test_chain_against_its_definition_and_adjoint():
    rng = np.random.default_rng(6)
    tex = rng.standard_normal((2, 16, 8, 3), dtype=f32)
    mip = mref.mipmaps(tex)
    l1, l2 = mref.level(tex, mip, 1), mref.level(tex, mip, 2)
    for (b, j, i, c) in ((0, 0, 0, 0), (1, 7, 3, 2), (0, 3, 1, 1)):
        want = ((tex[b, 2 * j, 2 * i, c] + tex[b, 2 * j, 2 * i + 1, c]) + (tex[b, 2 * j + 1, 2 * i, c] + tex[b, 2 * j + 1, 2 * i + 1, c])) * f32(0.25)
        assert l1[b, j, i, c] == want
    assert l2[1, 3, 1, 0] == ((l1[1, 6, 2, 0] + l1[1, 6, 3, 0]) + (l1[1, 7, 2, 0] + l1[1, 7, 3, 0])) * f32(0.25)
    assert np.array_equal(mref.mipmaps(tex, 1), mip[:, :32]) and mref.mipmaps(tex, 0).shape == (2, 0, 3)
    # the backward against the float64 sum: <g, mipmaps(t)> = <backward(g), t> for the linear map in float64, and texel by texel
    g = rng.standard_normal(mip.shape)
    t64 = rng.standard_normal(tex.shape)
    back = mref.mipmaps_backward64(tex.shape, None, g)
    lhs, rhs = (g * mref.mipmaps(t64, dtype=np.float64)).sum(), (back * t64).sum()
    assert abs(lhs - rhs) <= 1e-12 * np.abs(g).sum()
    _, levels, _ = mref.layout(16, 8)
    j, i = 13, 6
    want = sum(0.25 ** k * g[1, levels[k][2] + (j >> k) * levels[k][1] + (i >> k), 2] for k in range(1, 4))
    assert abs(back[1, j, i, 2] - want) < 1e-15


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("boundary_mode", mref.BOUNDARIES)
def test_grads64_against_finite_differences(boundary_mode, per_view):
    """grads64 is the derivative of the float32 function at its own float32 stage.  In (tex, mip) that function is linear: a
    directional difference of forward64 with the float32 fractions is exact up to float64 rounding.  In u (and v) it is piecewise
    linear, so a central difference of step 1e-6 of forward64 with exact fractions is exact where no tap's fraction lies within
    1e-3 of a texel's border (the kinks are left out) -- but its fractions differ from the float32 stage's by up to 2^-20 (half
    an ulp of |x| < 32), and du/dx is linear in fy with a slope of the size of du/dx itself: 2^-18 of the largest gradient."""
    size, C = (16, 8), 3
    rng = np.random.default_rng(7)
    uv, da, rl = mref.case(SHAPE, *size, seed=14)
    tex = rng.standard_normal(((2,) if per_view else ()) + size + (C,), dtype=f32)
    mip = mref.mipmaps(tex)
    g = rng.standard_normal(SHAPE + (C,), dtype=f32)
    dtex, dmip, duv = mref.grads64(uv, da, tex, mip, rl, boundary_mode, None, g)
    st = mref.stage(uv, da, *size, rl)
    assert dtex.shape == tex.shape and dmip.shape == mip.shape and np.abs(dtex).max() > 0 and np.abs(dmip).max() > 0
    assert not duv[st["empty"]].any()
    # (tex, mip): a random direction
    dt, dm = rng.standard_normal(tex.shape), rng.standard_normal(mip.shape)
    uv64 = np.where(st["empty"][..., None], 0.0, uv.astype(np.float64))
    base = mref.forward64(uv, da, tex, mip, rl, boundary_mode, st=st, stage_dtype=f32)
    moved = mref.forward64(uv, da, tex.astype(np.float64) + dt, mip.astype(np.float64) + dm, rl, boundary_mode, st=st, stage_dtype=f32)
    lhs, rhs = (g * (moved - base)).sum(), (dtex * dt).sum() + (dmip * dm).sum()
    assert abs(lhs - rhs) <= 1e-10 * (np.abs(dtex * dt).sum() + np.abs(dmip * dm).sum()), (lhs, rhs)
    # uv: central differences per slot (the slots are independent)
    h, margin = 1e-6, 1e-3
    away = ~st["empty"]
    for k in range(st["nlev"]):
        Hk, Wk = size[0] >> k, size[1] >> k
        used = (st["j"] == k) | (st["two"] & (st["j"] + 1 == k))
        x, y = uv64[..., 0] * Wk - 0.5, uv64[..., 1] * Hk - 0.5
        fx, fy = x - np.floor(x), y - np.floor(y)
        near = (np.minimum(fx, 1 - fx) < margin) | (np.minimum(fy, 1 - fy) < margin)
        away &= ~(used & near)
    assert away.sum() > 0.9 * (~st["empty"]).sum()
    for axis in range(2):
        e = np.zeros(2); e[axis] = h
        fd = (g * (mref.forward64(uv64 + e, da, tex, mip, rl, boundary_mode, st=st)
                   - mref.forward64(uv64 - e, da, tex, mip, rl, boundary_mode, st=st))).sum(-1) / (2 * h)
        err = np.abs(fd - duv[..., axis])[away]
        scale = np.abs(duv[..., axis][away]).max()
        assert scale > 0 and err.max() <= 2.0 ** -18 * scale, (axis, err.max(), scale)


def test_minified_checkerboard_is_grey():
    """What the feature is for: a 64 x 64 checkerboard of period two texels seen at about 8 texels per pixel.  Level 1 is exactly
    0.5 everywhere, so every slot with lod >= 1 returns exactly 0.5; the bilinear filter on the same input returns whatever
    four texels the sample falls between."""
    n = 64
    jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    tex = ((ii + jj) % 2).astype(f32)[..., None]
    mip = mref.mipmaps(tex)
    assert (mip == f32(0.5)).all() and mip.shape == ((4 ** 6 - 1) // 3, 1)
    rng = np.random.RandomState(8)
    shape = (1, 16, 16, 1)
    ys, xs = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    step = 8.0 / n                                                           # 8 texels per pixel
    uv = np.stack([xs * step, ys * step], -1).reshape(shape + (2,)) + rng.uniform(0, step, shape + (2,))   # jittered offsets
    uv = uv.astype(f32)
    da = np.broadcast_to(np.array([step, 0, 0, step], f32), shape + (4,)).copy()
    da *= rng.uniform(0.8, 1.25, shape + (1,)).astype(f32)
    st = mref.stage(uv, da, n, n)
    assert (st["lod"] >= 1).all() and not st["empty"].any()
    out = mref.forward32(uv, da, tex, mip)
    assert (out == f32(0.5)).all()
    lin = tref.forward32(uv, tex, None, "linear", "wrap")
    print("bilinear on the minified checkerboard spans", float(lin.min()), float(lin.max()))
    assert lin.max() - lin.min() > 0.5


# ---- the input sets of tests/test_gpu_texture_mip.py beyond ``case``: each held here to the condition its GPU test relies on ----

GRID_LS = (1, 3, 8)
GRID_TEXTURES = ((16, 8), (32, 32), (6, 10))


def test_keys_restate_the_forward():
    """The forward put together from ``keys`` alone (rows of tex and the chain stacked, texture_ref's fractions per level) is
    forward32, to the bit: the key space is the one the levels are read through."""
    size, C = (16, 8), 2
    uv, da, rl = mref.case(SHAPE, *size, seed=15)
    rng = np.random.default_rng(9)
    tex = rng.standard_normal(size + (C,), dtype=f32)
    mip = mref.mipmaps(tex)
    rows = np.concatenate([tex.reshape(-1, C), mip], 0)
    for boundary_mode in mref.BOUNDARIES:
        ks = mref.keys(uv, da, *size, rl, boundary_mode)
        st = mref.stage(uv, da, *size, rl)
        nlev, levels, T = mref.layout(*size)
        assert ks.shape == SHAPE + (8,) and ks.dtype == np.int64 and ks.max() < size[0] * size[1] + T
        assert (ks[st["empty"]] == -1).all() and (ks[~st["empty"]][:, :4] >= 0).all()
        assert ((ks[..., 4:] >= 0).all(-1) == st["two"]).all() and ((ks[..., 4:] == -1).all(-1) == ~st["two"]).all()
        out = np.zeros(SHAPE + (C,), f32)
        for k, (h, w, off) in enumerate(levels):
            lo, hi = (0, size[0] * size[1]) if k == 0 else (size[0] * size[1] + off, size[0] * size[1] + off + h * w)
            fr = tref.stage(uv, h, w, np.where(st["empty"], -1, 0), "linear", boundary_mode)
            for half, sel in ((0, ~st["empty"] & (st["j"] == k)), (1, st["two"] & (st["j"] + 1 == k))):
                kk = ks[..., 4 * half:4 * half + 4]
                assert ((kk[sel] >= lo) & (kk[sel] < hi)).all(), (k, half)
                t = rows[np.where(sel[..., None], kk, 0)]
                fx, fy = fr["fx"][..., None], fr["fy"][..., None]
                a, b = t[..., 0, :] + fx * (t[..., 1, :] - t[..., 0, :]), t[..., 2, :] + fx * (t[..., 3, :] - t[..., 2, :])
                c = a + fy * (b - a)
                if half == 0:
                    out = np.where(sel[..., None], c, out)
                else:
                    out = np.where(sel[..., None], out + st["f"][..., None] * (c - out), out)
        want = mref.forward32(uv, da, tex, mip, rl, boundary_mode)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), boundary_mode


@pytest.mark.parametrize("size", GRID_TEXTURES)
def test_grid_inputs_reach_every_branch(size):
    """``case`` at the channel and layer grid's shapes: every branch with one, three and eight layers."""
    nlev = mref.layout(*size)[0]
    for L in GRID_LS:
        uv, da, rl = mref.case((2, 20, 24, L), *size, seed=11)
        r = mref.reach(uv, da, *size, rl)
        print(size, L, r)
        assert r["magnified"] > 0 and r["beyond"] > 0 and r["empty_id"] > 0 and r["empty_uv"] > 0 and r["empty_da"] > 0
        assert len(r["pairs"]) == nlev - 1 and all(n > 0 for n in r["pairs"])
        st = mref.stage(uv, da, *size, rl)
        for l in range(L):                                                   # every layer has live slots: clear_keys runs between them
            assert (~st["empty"][..., l]).sum() > 100


def test_small_and_max_mip_level_inputs():
    for shape in ((1, 1, 1, 1), (2, 5, 3, 8), (1, 4, 5, 2)):
        uv, da, rl = mref.case(shape, 16, 8, seed=17)
        st = mref.stage(uv, da, 16, 8, rl)
        assert (~st["empty"]).sum() >= max(1, 0.8 * st["empty"].size), shape
        if st["empty"].size > 1:
            assert st["two"].any() and (~st["empty"] & ~st["two"]).any(), shape
    uv, da, rl = mref.case(SHAPE, 16, 8, seed=11)
    for mx, nlev in ((0, 1), (1, 2), (2, 3)):
        r = mref.reach(uv, da, 16, 8, rl, mx)
        assert len(r["pairs"]) == nlev - 1 and all(n > 100 for n in r["pairs"]) and r["beyond"] > 100 and r["magnified"] > 100, (mx, r)


def test_overflow_inputs_overflow_the_table():
    from util import table_capacity
    uv, da, rl = mref.overflow_case()
    size = mref.OVERFLOW_SIZE
    for layers in (None, rl):
        for boundary_mode in mref.BOUNDARIES:
            least = mref.distinct_keys_per_tile(uv, da, *size, layers, boundary_mode)
            print("distinct keys per tile and layer, at least", least, boundary_mode, layers is not None)
            assert least > 2 * table_capacity()
        r = mref.reach(uv, da, *size, layers)
        print(r)
        assert r["magnified"] > 100 and all(n > 100 for n in r["pairs"][:4])
    # both destination tensors in every tile: level 0's keys and the chain's
    ks = mref.keys(uv, da, *size, None, "wrap")
    B, H, W, L = mref.OVERFLOW_SHAPE
    for b in range(B):
        for y in range(0, H, 16):
            for x in range(0, W, 16):
                k = np.unique(ks[b, y:y + 16, x:x + 16])
                k = k[k >= 0]
                assert (k < size[0] * size[1]).sum() > table_capacity() // 2 and (k >= size[0] * size[1]).sum() > table_capacity() // 2


def test_hot_inputs_share_a_few_keys():
    uv, da = mref.hot_case_magnified()
    st = mref.stage(uv, da, 8, 8)
    assert not st["empty"].any() and (st["lod"] <= 0).all()
    most = mref.distinct_keys_per_tile(uv, da, 8, 8, worst=max)
    print("magnified: distinct keys per tile and layer, at most", most)
    assert 0 < most <= 16
    for size, top in (((8, 8), 1), ((16, 8), 2)):
        uv, da = mref.hot_case_beyond(*size)
        st = mref.stage(uv, da, *size)
        nlev, levels, T = mref.layout(*size)
        assert not st["empty"].any() and not st["two"].any() and (st["lod"] >= nlev - 1).all() and (st["j"] == nlev - 1).all()
        assert (st["lod"] == 64).mean() > 1 / 16 and np.isfinite(da).all()
        for boundary_mode in mref.BOUNDARIES:
            ks = mref.keys(uv, da, *size, None, boundary_mode)
            first = size[0] * size[1] + levels[-1][2]
            assert (ks[..., 4:] == -1).all() and (ks[..., :4] >= first).all() and (ks[..., :4] < first + top).all()
            assert mref.distinct_keys_per_tile(uv, da, *size, None, boundary_mode, worst=max) == top
            assert mref.distinct_keys_per_tile(uv, da, *size, None, boundary_mode) == top


@pytest.mark.parametrize("size,mx", mref.EDGE_TEXTURES)
def test_lod_edge_table_reaches_every_edge(size, mx):
    """What ``lod_edge_footprints`` reaches by ``stage``: each branch point of the level of detail exactly, and a strict
    neighbour on each side of it."""
    uv, da = mref.lod_edge_case(*size, mx)
    st = mref.stage(uv, da, *size, None, mx)
    lod, r2 = mref.lod32(da, *size)
    nlev = st["nlev"]
    assert nlev >= 2 and not st["empty"].any() and len(mref.lod_edge_footprints(*size, mx)) <= 128
    one = f32(1)
    # r2 > 1 against r2 == 1, lod <= 0
    assert ((r2 == one) & (lod == 0) & ~st["two"] & (st["j"] == 0)).sum() >= 2
    assert (r2 == np.nextafter(one, f32(0))).any() and (r2 == np.nextafter(one, f32(2))).any()
    assert ((r2 > one) & (lod > 0) & (lod < f32(1e-6)) & st["two"] & (st["j"] == 0)).any()
    assert (r2 == 0).sum() >= 4 and ((r2 > 0) & (r2 < one)).any()
    # an integer lod between the ends: two levels, f == 0
    for k in range(1, nlev - 1):
        kf = f32(k)
        assert (st["two"] & (st["f"] == 0) & (st["j"] == k) & (lod == kf)).sum() >= 2, k
        assert (lod == np.nextafter(kf, f32(0))).any() and (lod == np.nextafter(kf, f32(99))).any(), k
        assert (r2 == np.nextafter(f32(4.0 ** k), f32(0))).any() and (r2 == np.nextafter(f32(4.0 ** k), f32(1e9))).any(), k
    # lod >= nlev - 1: exactly there one level, the float below it two
    top = f32(nlev - 1)
    assert ((lod == top) & ~st["two"] & (st["j"] == nlev - 1)).sum() >= 2
    below = lod == np.nextafter(top, f32(0))
    assert below.any() and (st["two"] & (st["j"] == nlev - 2))[below].all() and (st["f"][below] > f32(0.999)).all()
    assert ((lod > top) & (lod < top + f32(1e-5)) & ~st["two"]).any()
    assert (lod == f32(nlev)).any()                                           # the k = nlev rows: a whole level beyond
    # r2 = inf
    assert (np.isinf(r2) & (lod == 64) & (st["j"] == nlev - 1)).sum() >= 4
    # either axis the larger, both signs
    with np.errstate(over="ignore"):
        sx = (da[..., 0] * f32(size[1])) ** 2 + (da[..., 1] * f32(size[0])) ** 2
        sy = (da[..., 2] * f32(size[1])) ** 2 + (da[..., 3] * f32(size[0])) ** 2
        assert ((sy > sx) & (lod > 0)).any() and ((sx > sy) & (lod > 0)).any() and (da < 0).any() and np.signbit(da[da == 0]).any()
    # every row of the table meets several uv
    assert np.prod(mref.EDGE_SHAPE) >= 4 * len(mref.lod_edge_footprints(*size, mx))


def test_lattice_inputs_sit_on_centres_and_borders():
    """The lattice's fractions are exact at every level (multiples of 1/32; on level 0's rows, 16 high, 0 or 0.5 alone), with 0
    (a texel centre: floorf alone decides the tap) and 0.5 (a texel border) on both axes of every level; u and v exactly 0 and 1
    and negative; ``outside`` puts every tap of every level beyond the border; the range rule's slots are live and empty as
    RANGE_EDGES says."""
    Ht, Wt = mref.LATTICE_SIZE
    nlev, levels, _ = mref.layout(Ht, Wt)
    seen = set()
    for scale, want_j, want_two in zip(mref.LATTICE_SCALES, (0, 0, 1, 2, 3), (False, True, True, True, False)):
        uv, da = mref.lattice_case(scale)
        st = mref.stage(uv, da, Ht, Wt)
        assert not st["empty"].any() and (st["j"] == want_j).all() and (st["two"] == want_two).all(), scale
        if want_two:
            assert (st["f"] == f32(0.5)).all()
        seen |= {want_j} | ({want_j + 1} if want_two else set())
    assert seen == set(range(nlev))
    uv, _ = mref.lattice_case(1.0)
    k32 = np.round(uv.astype(np.float64) * 32).astype(np.int64)
    assert np.array_equal(k32 / 32.0, uv) and k32.min() == -40 and k32.max() == 72
    for axis in range(2):
        assert (uv[..., axis] == 0).any() and (uv[..., axis] == 1).any() and (uv[..., axis] < 0).any() and (uv[..., axis] > 1).any()
    for h, w, _ in levels:
        s = tref.stage(uv, h, w, None, "linear", "wrap")
        for axis, n, fr in ((0, w, s["fx"]), (1, h, s["fy"])):
            exact = k32[..., axis] * n / 32.0 - 0.5                          # (exact in float64)
            assert np.array_equal(fr.astype(np.float64), exact - np.floor(exact)), (h, w, axis)
            assert (fr == 0).sum() > 50 and (fr == f32(0.5)).sum() > 50, (h, w, axis)
            if n == 16:
                assert np.isin(fr, (0, 0.5)).all()
        if h == 1 or w == 1:                                                 # an extent of 1 under wrap: negative remainders
            assert (np.floor(s["x" if w == 1 else "y"]) < 0).sum() > 50
    uvo, _ = mref.lattice_case(1.0, outside=True)
    for h, w, off in levels:
        idx = tref.stage(uvo, h, w, None, "linear", "clamp")["idx"]
        corners = [0, w - 1, (h - 1) * w, h * w - 1]
        assert (idx == idx[..., :1]).all() and np.isin(idx, corners).all() and set(np.unique(idx)) == set(corners)
    uvr, live = mref.range_case(uv)
    e = tref.empty(uvr, Ht, Wt)
    assert np.array_equal(~e[0, 0, :5].reshape(-1), live) and np.array_equal(~e[0, 1, :5].reshape(-1), live) and live[0] and not live[1:4].any()
    s = tref.stage(uvr, Ht, Wt, None, "linear", "wrap")
    assert s["x"][0, 0, 0, 0] == f32(2.0 ** 24 - 2) and s["y"][0, 1, 0, 0] == f32(2.0 ** 24 - 2)     # the largest a slot can have
    assert e.sum() == 2 * (~live).sum()


def test_instantiation_inputs_are_what_they_are_for():
    """The inputs of test_gpu_texture_mip.py's test_every_instantiation_once: every tile has live and empty slots in both
    layers, slots in each of the three level-of-detail cases, and taps in both destination tensors (tex and the chain)."""
    uv, da, rl = mref.instantiation_case()
    Ht, Wt = mref.INST_TEXTURE
    st = mref.stage(uv, da, Ht, Wt, rl)
    assert st["nlev"] == 3 and tref.tiles_have_live_and_empty(st["empty"])
    live = ~st["empty"]
    low, high = live & (st["lod"] <= 0), live & (st["lod"] >= st["nlev"] - 1)
    print("lod <= 0:", int(low.sum()), "two levels:", int(st["two"].sum()), "top level:", int(high.sum()))
    assert min(low.sum(), st["two"].sum(), high.sum()) >= 20 and low.sum() + st["two"].sum() + high.sum() == live.sum()
    assert set(np.unique(st["j"][st["two"]])) == {0, 1}                                # both pairs of levels blend
    bad_uv, bad_da = ~np.isfinite(uv).all(-1), ~np.isfinite(da).all(-1)
    assert bad_uv.sum() == 6 and bad_da.sum() == 4 and np.array_equal(st["empty"], (rl < 0) | bad_uv | bad_da)
    for boundary_mode in mref.BOUNDARIES:
        k = mref.keys(uv, da, Ht, Wt, rl, boundary_mode)
        assert ((k >= 0) & (k < Ht * Wt)).any() and (k >= Ht * Wt).any()
