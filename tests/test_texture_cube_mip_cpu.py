"""The numpy restatement of the cube mip chain's contract (tests/texture_cube_mip_ref.py), pinned without the kernels: the
clamped ends and the integer levels against the cube op's restatement; constant cubes; edges seen from both faces at every
level size; the gradients, the level's among them, against float64 central differences; the box chain; what the feature is for
(a checkerboard cube is flat at level 1); and the interface the feature adds."""
import inspect

import numpy as np
import pytest

import texture_cube_mip_ref as ref
import texture_cube_ref as cref
import texture_mip_ref as mref
from util import assert_own_exports

U32 = 2.0 ** -24                    # unit roundoff of float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _as_slots(d):
    return np.asarray(d).reshape(1, 1, -1, 1, 3)


def _dirs(rng, n, N, dtype=np.float32):
    """n random directions and 2 (n // 4) near_seams ones at this face size, as (1, 1, *, 1, 3)."""
    d = np.concatenate([rng.standard_normal((n, 3)) * np.exp(rng.uniform(-2, 2, (n, 1))), cref.near_seams(rng, n // 4, N)])
    return _as_slots(d).astype(dtype)


def _cube(rng, N, C, max_mip_level=None, B=None):
    tex = rng.standard_normal(((B,) if B else ()) + (6, N, N, C)).astype(np.float32)
    return tex, ref.box_chain(tex, max_mip_level)


@pytest.mark.parametrize("N,max_mip_level", [(1, None), (2, None), (4, None), (5, None), (6, None), (8, None), (8, 1), (8, 0)])
def test_clamped_ends_and_integer_levels_are_single_levels(N, max_mip_level):
    rng = np.random.default_rng(1)
    tex, mip = _cube(rng, N, 3, max_mip_level)
    mip = rng.standard_normal(mip.shape).astype(np.float32)               # (any chain: not the box chain)
    nlev, levels, T = ref.layout(N, max_mip_level)
    assert mip.shape == (6, T, 3)
    d = _dirs(rng, 3000, N)
    shape = d.shape[:4]
    for lod in (0.0, -0.0, -1.5, -1e30):
        got = ref.forward32(d, np.full(shape, lod, np.float32), tex, mip, None, max_mip_level)
        assert np.array_equal(_bits(got), _bits(cref.forward32(d, tex))), (N, lod)
    for k in range(nlev):                                                 # an integer level: f = 0, c_k + 0 (c_{k+1} - c_k)
        got = ref.forward32(d, np.full(shape, k, np.float32), tex, mip, None, max_mip_level)
        assert np.array_equal(_bits(got), _bits(cref.forward32(d, ref.level_cube(tex, mip, k, max_mip_level)))), (N, k)
    last = cref.forward32(d, ref.level_cube(tex, mip, nlev - 1, max_mip_level))
    for lod in (nlev - 1, nlev - 0.5, nlev + 3.0, 1e30):
        got = ref.forward32(d, np.full(shape, lod, np.float32), tex, mip, None, max_mip_level)
        assert np.array_equal(_bits(got), _bits(last)), (N, lod)
    for lod in (np.nan, np.inf, -np.inf):                                 # empty slots
        got = ref.forward32(d, np.full(shape, lod, np.float32), tex, mip, None, max_mip_level)
        assert not got.any()


def test_constant_cube():
    """Every texel of every level c.  Four taps at both levels: c_k = c exactly and c + f (c - c) = c.  With a corner sample
    at either level |c_k - c| <= 9 u |c| (tests/test_texture_cube_cpu.py::test_constant_cube); the blend is a convex combination
    of the two, within 9 u |c|, plus the rounding of its last addition, u (1 + 9 u) |c|: |out - c| < 11 u |c|."""
    N = 4
    rng = np.random.default_rng(2)
    d = _dirs(rng, 6000, 2)
    lod = rng.uniform(-1, 4, d.shape[:4]).astype(np.float32)
    st = ref.stage(d, lod, N)
    corner = np.zeros(d.shape[:4], bool)
    for k, sk in ref.level_stages(d, st, N).items():
        corner |= sk["miss"] >= 0
    assert corner.sum() > 200 and (~corner).sum() > 2000 and st["two"].sum() > 2000
    for c in (3.25, -1e-3, 7e5):
        tex = np.full((6, N, N, 2), c, np.float32)
        mip = np.full((6, 5, 2), c, np.float32)
        cf = float(np.float32(c))
        out = ref.forward32(d, lod, tex, mip).astype(np.float64)
        assert (out[~corner] == cf).all()
        assert np.abs(out[corner] - cf).max() <= 11 * U32 * abs(cf)


def _named(st, k, N, lvl):
    """{key: weight} of slot k of a (1, 1, n, 1) cube stage at level ``lvl``, weights on one key added."""
    w = cref.tap_weights(st)[0, 0, k, 0]
    keys = ref.level_keys(st["idx"][0, 0, k, 0], N, lvl)
    out = {}
    for t, wk, has in zip(keys, w, np.arange(4) != st["miss"][0, 0, k, 0]):
        if has and wk != 0:
            out[int(t)] = out.get(int(t), 0.0) + float(wk)
    return out


def test_on_edge_directions_name_the_same_keys_from_both_faces_at_every_level():
    """tests/test_texture_cube_cpu.py's edge walk at the level sizes 4, 2 and 1 of an N = 4 cube, in the op's key space."""
    N = 4
    nlev, levels, T = ref.layout(N)
    assert [l[0] for l in levels] == [4, 2, 1] and T == 5
    us = np.array([-1.0, -0.875, -0.625, -0.5, -0.125, 0.0, 0.25, 0.375, 0.75, 0.875, 1.0])
    for lvl in range(nlev):
        Nk = N >> lvl
        seen, lo, hi = set(), 6 * N * N + 6 * T, -1
        for f in range(6):
            for e in range(4):
                g = cref.SEAMS[f][e][0]
                fixed = -1.0 if e % 2 == 0 else 1.0
                pts = np.array([cref._point(f, fixed, u) if e < 2 else cref._point(f, u, fixed) for u in us])
                d = _as_slots(pts).astype(np.float32)
                a = cref.stage(d, Nk, None, "linear", face=np.full(d.shape[:4], f))
                b = cref.stage(d, Nk, None, "linear", face=np.full(d.shape[:4], g))
                for k in range(len(us)):
                    na, nb = _named(a, k, N, lvl), _named(b, k, N, lvl)
                    assert set(na) == set(nb), (lvl, f, e, us[k], na, nb)
                    assert all(abs(na[t] - nb[t]) <= 1e-12 for t in na), (lvl, f, e, us[k])
                    lo, hi = min(lo, *na), max(hi, *na)
                seen.add(frozenset(((f, e), (g, cref.SEAMS[f][e][1]))))
        assert len(seen) == 12
        # the keys of a level stay in its own range of the key space
        first = 0 if lvl == 0 else 6 * N * N + levels[lvl][2]
        assert lo >= first and hi < (6 * N * N if lvl == 0 else 6 * N * N + 5 * T + levels[lvl][2] + Nk * Nk)


MARGIN = 5e-4                       # texels (and levels) a sample keeps from every floor jump


def _fd_set(rng, N, B):
    """(dirs (B,2,n,3,3) float64, level (B,2,n,3) float64, excluded share): random and near-seam directions at every level
    size, levels in [-1, nlev + 1]; dropped: samples within MARGIN of a texel border or a face switch at a level they use, or
    of an integer level."""
    nlev = ref.layout(N)[0]
    cand = np.concatenate([rng.standard_normal((3000, 3)) * np.exp(rng.uniform(-2, 2, (3000, 1)))]
                          + [cref.near_seams(rng, 500, N >> k) for k in range(nlev)])
    cand = _as_slots(rng.permutation(cand))
    lod = rng.uniform(-1, nlev + 1, cand.shape[:4])
    st = ref.stage(cand, lod, N, None, None, np.float64)
    ok = np.abs(lod - np.round(lod)) > MARGIN
    for k, sk in ref.level_stages(cand, st, N, np.float64).items():
        used = ~sk["empty"]
        for f, x in ((sk["fx"], sk["x"]), (sk["fy"], sk["y"])):
            ok &= ~used | ((f >= MARGIN) & (f <= 1 - MARGIN) & (x >= -0.5 + MARGIN) & (x <= (N >> k) - 0.5 - MARGIN))
    ok = ok[0, 0, :, 0]
    n = (int(ok.sum()) // (B * 6)) * B * 6
    keep = np.flatnonzero(ok)[:n]
    return cand[0, 0, keep, 0].reshape(B, 2, -1, 3, 3), lod[0, 0, keep, 0].reshape(B, 2, -1, 3), 1.0 - ok.mean()


@pytest.mark.parametrize("per_view", (False, True))
def test_grads64_against_central_differences(per_view):
    N, B, C = 4, 2, 2
    rng = np.random.default_rng(5)
    d, lod, excluded = _fd_set(rng, N, B)
    print("excluded share", excluded)
    assert excluded < 0.01
    shape = d.shape[:4]
    nlev, levels, T = ref.layout(N)
    tex = rng.standard_normal(((B,) if per_view else ()) + (6, N, N, C))
    mip = rng.standard_normal(((B,) if per_view else ()) + (6, T, C))      # not the box chain
    rl = rng.integers(-1, 3, shape).astype(np.int32)
    g = rng.standard_normal(shape + (C,))
    st = ref.stage(d, lod, N, rl, None, np.float64)
    stages = ref.level_stages(d, st, N, np.float64)
    for which in ("first", "second"):                                     # corner, seam and interior samples at both levels
        corner = seam = inner = 0
        for k, sk in stages.items():
            first, second = ref._users(st, k)
            m = (first & st["two"]) if which == "first" else second
            corner += int((m & (sk["miss"] >= 0)).sum())
            seam += int((m & sk["seam"].any(-1) & (sk["miss"] < 0)).sum())
            inner += int((m & ~sk["seam"].any(-1) & (sk["miss"] < 0)).sum())
        assert corner > 50 and seam > 50 and inner > 50, (which, corner, seam, inner)
    assert (~st["two"] & ~st["empty"]).sum() > 100
    dtex, dmip, ddir, dlevel, _ = ref.grads64(d, lod, tex, mip, rl, None, g, stage_dtype=np.float64)

    def slot_loss(d_, lod_, tex_, mip_):
        return (ref.forward64(d_, lod_, tex_, mip_, rl) * g).sum(-1)
    base = slot_loss(d, lod, tex, mip).sum()
    for name, t, want in (("tex", tex, dtex), ("mip", mip, dmip)):         # linear in both: a unit step is exact
        assert np.abs(want).max() > 0
        if per_view:                                                      # (element by element for the shared cube; here 24 random steps)
            for _ in range(24):
                p = rng.standard_normal(t.shape)
                moved = (slot_loss(d, lod, tex + p, mip).sum() if name == "tex" else slot_loss(d, lod, tex, mip + p).sum()) - base
                assert abs(moved - (want * p).sum()) <= 1e-10 * np.abs(want * p).sum(), name
            continue
        fd = np.zeros_like(t)
        for k in range(t.size):
            p = t.copy()
            p.reshape(-1)[k] += 1.0
            fd.reshape(-1)[k] = (slot_loss(d, lod, p, mip).sum() if name == "tex" else slot_loss(d, lod, tex, p).sum()) - base
        assert np.abs(fd - want).max() <= 1e-10 * np.abs(want).max(), name
    # a step of 1e-6 moves a sample by < 3 N / 2 * 1e-6 / |dir| < 5e-5 texels (|dir| >= e^-2), inside the margin
    h = 1e-6
    fd = np.zeros_like(d)
    for k in range(3):
        p, m = d.copy(), d.copy()
        p[..., k] += h
        m[..., k] -= h
        fd[..., k] = (slot_loss(p, lod, tex, mip) - slot_loss(m, lod, tex, mip)) / (2 * h)
    assert np.abs(ddir).max() > 0 and np.abs(fd - ddir).max() <= 1e-6 * np.abs(ddir).max()
    assert (ddir[rl < 0] == 0).all() and (dlevel[rl < 0] == 0).all()
    dot = (ddir * d).sum(-1)
    assert np.abs(dot).max() <= 1e-12 * (np.abs(ddir) * np.abs(d)).sum(-1).max()
    # the level: piecewise linear in lod, so the central difference is exact up to rounding
    h = 1e-5
    fd = (slot_loss(d, lod + h, tex, mip) - slot_loss(d, lod - h, tex, mip)) / (2 * h)
    assert np.abs(dlevel).max() > 0 and np.abs(fd - dlevel).max() <= 1e-8 * np.abs(dlevel).max()
    assert (dlevel[~st["two"]] == 0).all() and (dlevel[st["two"]] != 0).mean() > 0.99


def test_integer_level_takes_the_right_hand_derivative():
    N = 4
    rng = np.random.default_rng(6)
    tex, mip = _cube(rng, N, 2)
    d = _dirs(rng, 500, N)
    g = rng.standard_normal(d.shape[:4] + (2,))
    lod = np.ones(d.shape[:4], np.float32)
    *_, dlevel, _ = ref.grads64(d, lod, tex, mip, None, None, g)
    c1 = cref.forward64(d, ref.level_cube(tex, mip, 1))
    c2 = cref.forward64(d, ref.level_cube(tex, mip, 2))
    assert np.abs(dlevel - (g * (c2 - c1)).sum(-1)).max() <= 1e-5 * np.abs(dlevel).max()
    for clamped in (0.0, 2.0, -1.0, 5.0):                                  # at and beyond the ends: no gradient
        *_, dl, _ = ref.grads64(d, np.full(d.shape[:4], clamped, np.float32), tex, mip, None, None, g)
        assert not dl.any()


@pytest.mark.parametrize("N,max_mip_level", [(8, None), (8, 1), (6, None), (5, None)])
def test_box_chain_is_the_mipmaps_of_each_face(N, max_mip_level):
    rng = np.random.default_rng(7)
    tex = rng.standard_normal((2, 6, N, N, 3)).astype(np.float32)
    chain = ref.box_chain(tex, max_mip_level)
    nlev, levels, T = ref.layout(N, max_mip_level)
    assert chain.shape == (2, 6, T, 3) and (nlev, T) == mref.layout(N, N, max_mip_level)[::2]
    for b in range(2):
        for f in range(6):
            assert np.array_equal(_bits(chain[b, f]), _bits(mref.mipmaps(tex[b, f], max_mip_level)))
    assert np.array_equal(_bits(ref.box_chain(tex[0], max_mip_level)), _bits(chain[0]))
    if N == 8 and max_mip_level is None:                                  # the 1 x 1 level is the face mean
        top = ref.level_cube(tex, chain, 3)
        assert top.shape == (2, 6, 1, 1, 3)
        assert np.abs(top[:, :, 0, 0] - tex.astype(np.float64).mean((2, 3))).max() <= 8 * U32 * np.abs(tex).max()


def test_checkerboard_cube_is_flat_at_level_one():
    """What the feature is for: faces that alternate 0 and 1 from texel to texel.  "linear" (and level 0) swings over the whole
    range with the direction; level 1 is the 2 x 2 mean, 0.5 on every face, so every sample of it, seams and corners included,
    is exactly 0.5."""
    N = 4
    jj, ii = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    tex = np.broadcast_to(((ii + jj) % 2).astype(np.float32)[None, :, :, None], (6, N, N, 1)).copy()
    mip = ref.box_chain(tex)
    assert (ref.level_cube(tex, mip, 1) == 0.5).all()
    rng = np.random.default_rng(0)
    d = _as_slots(np.concatenate([rng.standard_normal((5000, 3)), cref.near_seams(rng, 500, 2)])).astype(np.float32)
    st = cref.stage(d, 2, None, "linear")
    assert (st["miss"] >= 0).sum() > 100 and st["seam"].any(-1).sum() > 300
    one = ref.forward32(d, np.ones(d.shape[:4], np.float32), tex, mip)
    assert one.min() == 0.5 and one.max() == 0.5
    zero = ref.forward32(d, np.zeros(d.shape[:4], np.float32), tex, mip)
    assert np.array_equal(_bits(zero), _bits(cref.forward32(d, tex)))
    assert zero.min() < 0.01 and zero.max() > 0.99
    half = ref.forward32(d, np.full(d.shape[:4], 0.5, np.float32), tex, mip)      # half way: half the swing
    assert np.abs(half - 0.5).max() <= 0.25 + 1e-6


def test_keys_and_level_edges():
    N = 4
    rng = np.random.default_rng(8)
    d = _dirs(rng, 2000, N)
    lod = rng.uniform(-1, 4, d.shape[:4]).astype(np.float32)
    ks = ref.keys(d, lod, N)
    st = ref.stage(d, lod, N)
    T = ref.layout(N)[2]
    assert ks.max() < 6 * (N * N + T) and (ks[~st["two"]][:, 4:] == -1).all()
    assert ((ks[st["two"]] >= 0).sum(-1) >= 6).all()                      # at most one missing tap per level
    lvl0 = st["j"] == 0
    assert (ks[lvl0][:, :4] < 6 * N * N).all() and (ks[st["j"] > 0][:, :4][ks[st["j"] > 0][:, :4] >= 0] >= 6 * N * N).all()
    e = ref.level_edges(3)
    assert np.isnan(e).sum() == 1 and np.isinf(e).sum() == 2 and {0.0, 1.0, 2.0, 3.0} <= set(e[np.isfinite(e)].tolist())
    se = ref.stage(np.ones((1, 1, len(e), 1, 3), np.float32), e.reshape(1, 1, -1, 1), N)
    assert se["empty"].sum() == 3 and set(se["j"][~se["empty"]].tolist()) == {0, 1, 2} and se["two"].sum() >= 5


def test_interface():
    """Fails without the feature: the two exports, the two wrappers, the autograd function, the keyword; CPU tensors are
    refused like everywhere else; mip_level with another mode combination is a ValueError naming it."""
    import torch

    import dmesh2_renderer_amd as dm2
    from dmesh2_renderer_amd import _C
    assert_own_exports("dm2_texture_cube_mip")                           # its own two symbols, no boundary code
    assert "cube" not in _C.TEX_BOUNDARIES
    assert callable(_C.texture_cube_mip_cuda) and callable(_C.texture_cube_mip_backward_cuda)
    assert "TextureCubeMipFunction" in dm2.__all__ and issubclass(dm2.TextureCubeMipFunction, torch.autograd.Function)
    params = list(inspect.signature(dm2.Renderer.texture).parameters)
    assert params[-1] == "mip_level" and params[-4:-1] == ["uv_da", "mip", "max_mip_level"]
    assert dm2.LayeredRenderer.texture is dm2.Renderer.texture
    d = torch.ones((1, 2, 3, 2, 3))
    lod = torch.ones((1, 2, 3, 2))
    tex, mip = torch.zeros((6, 4, 4, 3)), torch.zeros((6, 5, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_cube_mip_cuda(d, lod, tex, mip)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.texture_cube_mip_backward_cuda(d, lod, tex, mip, None, None, torch.ones((1, 2, 3, 2, 3)), True, True, True, True)
    # (the checks of the modes come before anything touches the renderer or a device)
    for kw in (dict(), dict(filter_mode="linear-mipmap-linear"), dict(boundary_mode="clamp"), dict(filter_mode="nearest", boundary_mode="cube"),
               dict(filter_mode="linear", boundary_mode="cube")):
        with pytest.raises(ValueError, match="mip_level"):
            dm2.Renderer.texture(None, d, tex, mip_level=lod, **kw)
    with pytest.raises(ValueError, match="boundary_mode"):
        dm2.Renderer.texture(None, d, tex, filter_mode="linear-mipmap-linear", boundary_mode="cube", uv_da=torch.zeros((1, 2, 3, 2, 4)),
                             mip_level=lod)
    with pytest.raises(ValueError, match="boundary_mode"):
        dm2.Renderer.texture(None, d, tex, filter_mode="linear-mipmap-linear", boundary_mode="cube")
