"""The numpy restatement of the cube-map contract (tests/texture_cube_ref.py), pinned without the kernels: its seam table,
derived from the cube's geometry, against the literal the kernel carries; the interior of a face against the 2D op's
restatement; constant cubes; directions exactly on an edge seen from both faces; continuity across edges and corners; the
gradients against float64 central differences; scale invariance, mass, empty slots and ties."""
import os
import re

import numpy as np
import pytest

import texture_cube_ref as ref
import texture_ref as ref2d
from util import ROOT

U32 = 2.0 ** -24                    # unit roundoff of float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _as_slots(d):
    """(n, 3) directions as a (1, 1, n, 1, 3) slot tensor."""
    d = np.asarray(d)
    return d.reshape(1, 1, -1, 1, 3)


def _dirs(rng, n, dtype=np.float32):
    return _as_slots(rng.standard_normal((n, 3)) * np.exp(rng.uniform(-2, 2, (n, 1)))).astype(dtype)


def _near_seams(rng, n, N, reach=0.6):
    return _as_slots(ref.near_seams(rng, n, N, reach))


def test_seam_table_equals_the_kernels_literal():
    src = open(os.path.join(ROOT, "dmesh2_renderer_amd", "csrc", "dm2_texture_cube.hip")).read()
    body = re.search(r"CUBE_SEAM\[6\]\[4\]\[3\] = \{(.*?)\};", src, flags=re.S).group(1)
    nums = [int(x) for x in re.findall(r"-?\d+", body)]
    assert len(nums) == 72
    literal = tuple(tuple(tuple(nums[(f * 4 + e) * 3:(f * 4 + e) * 3 + 3]) for e in range(4)) for f in range(6))
    assert literal == ref.seam_table()
    # the table is an involution: across the edge and back is the same border, with the same reversal
    for f in range(6):
        for e in range(4):
            g, ne, rev = literal[f][e]
            assert literal[g][ne] == (f, e, rev) and g // 2 != f // 2


@pytest.mark.parametrize("N", (1, 2, 5, 64))
def test_interior_is_the_2d_op(N):
    rng = np.random.default_rng(1)
    d = _dirs(rng, 20_000)
    tex = rng.standard_normal((6, N, N, 3), dtype=np.float32)
    st = ref.stage(d, N, None, "linear")
    inside = ~st["seam"].any(-1) & (st["miss"] < 0)
    got = ref.forward32(d, tex)
    f32 = np.float32
    with np.errstate(invalid="ignore"):
        s = (f32(0.5) * ((st["sc"] / st["ma"]).astype(f32) + f32(1))).astype(f32)
        t = (f32(0.5) * ((st["tc"] / st["ma"]).astype(f32) + f32(1))).astype(f32)
    uv = np.stack([s, t], -1)
    n = 0
    for f in range(6):
        m = inside & (st["face"] == f)
        if N > 2:
            assert m.sum() > 100, (N, f)
        want = ref2d.forward32(uv, tex[f], None, "linear", "clamp")
        assert np.array_equal(_bits(got[m]), _bits(want[m])), (N, f)
        n += int(m.sum())
    assert n == inside.sum() and (N <= 2 or n > 5000) and (N != 1 or n == 0)


@pytest.mark.parametrize("N", (1, 2, 5))
@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_constant_cube(N, filter_mode):
    """With every texel c: a = c + fx (c - c) = c exactly, so a sample with four taps is c to the bit.  At a corner
    out = fl(sum_k w_k c) / fl(sum_k w_k): three roundings of products and three of sums above (relative (1 + u)^4 on every
    term), three of sums below, one of the division: |out - c| <= ((1 + u)^8 - 1) |c| < 9 u |c|, u = 2^-24."""
    rng = np.random.default_rng(2)
    d = np.concatenate([_dirs(rng, 5000), _near_seams(rng, 2000, N).astype(np.float32)], 2)
    for c in (3.25, -1e-3, 7e5):
        tex = np.full((6, N, N, 2), c, np.float32)
        cf = float(np.float32(c))
        out = ref.forward32(d, tex, None, filter_mode).astype(np.float64)
        st = ref.stage(d, N, None, filter_mode)
        corner = st["miss"] >= 0
        assert not st["empty"].any()
        assert (out[~corner] == cf).all()
        if filter_mode == "linear":
            assert corner.sum() > 200 and st["seam"].any(-1).sum() > 1000
            assert np.abs(out[corner] - cf).max() <= 9 * U32 * abs(cf)


def _named(st, k):
    """{texel: weight} of slot k of a (1, 1, n, 1) stage, zero weights dropped, weights on one texel added."""
    w = ref.tap_weights(st)[0, 0, k, 0]
    out = {}
    for t, wk, has in zip(st["idx"][0, 0, k, 0], w, np.arange(4) != st["miss"][0, 0, k, 0]):
        if has and wk != 0:
            out[int(t)] = out.get(int(t), 0.0) + float(wk)
    return out


@pytest.mark.parametrize("N", (1, 2, 5))
def test_on_edge_directions_name_the_same_texels_from_both_faces(N):
    """A direction exactly on a cube edge (|sc| == ma: fx == 0.5 exactly), evaluated as either adjacent face through stage's
    face override, on all 12 edges (each from both of its faces: 24 (face, border) pairs).  The positions along the edge are
    multiples of 1/8, so every fraction is exact in float32 and a reversed edge gives 1 - f exactly."""
    seen_edges, corners = set(), 0
    us = np.array([-1.0, -0.875, -0.625, -0.5, -0.125, 0.0, 0.25, 0.375, 0.75, 0.875, 1.0])
    for f in range(6):
        for e in range(4):
            g = ref.SEAMS[f][e][0]
            fixed = -1.0 if e % 2 == 0 else 1.0
            pts = np.array([ref._point(f, fixed, u) if e < 2 else ref._point(f, u, fixed) for u in us])
            d = _as_slots(pts * np.array([0.25, 1.0, 4.0, 1.0, 0.5, 2.0, 1.0, 8.0, 1.0, 0.125, 1.0])[:, None]).astype(np.float32)
            shape = d.shape[:4]
            a = ref.stage(d, N, None, "linear", face=np.full(shape, f))
            b = ref.stage(d, N, None, "linear", face=np.full(shape, g))
            assert (a["fx" if e < 2 else "fy"] == 0.5).all()
            for k in range(len(us)):
                na, nb = _named(a, k), _named(b, k)
                assert set(na) == set(nb), (N, f, e, us[k], na, nb)
                assert all(abs(na[t] - nb[t]) <= 1e-12 for t in na), (N, f, e, us[k], na, nb)
                assert abs(sum(na.values()) - 1.0) <= 1e-12
            corners += int((a["miss"] >= 0).sum())
            seen_edges.add(frozenset(((f, e), (g, ref.SEAMS[f][e][1]))))
            # and the samples are the same numbers
            tex = np.random.default_rng(3).standard_normal((6, N, N, 2), dtype=np.float32)
            oa = ref.forward64(d, tex, None, "linear", face=np.full(shape, f))
            ob = ref.forward64(d, tex, None, "linear", face=np.full(shape, g))
            assert np.abs(oa - ob).max() <= 1e-12
    assert len(seen_edges) == 12 and corners >= 48


@pytest.mark.parametrize("N", (1, 2, 5, 16))
def test_continuity_across_edges_and_corners(N):
    """Two directions an angle theta apart differ in the sample by no more than 4 sqrt(2) N R theta, R = max - min of the cube.

    Derivation.  Inside a bilinear cell |d out / d x| <= R.  At a corner out = sum_k w_k t_k / W and d out / d fx =
    sum_k (dw_k / dfx) (t_k - out) / W with sum_k |dw_k / dfx| <= 2 over the taps that exist, |t_k - out| <= R and W >= 3/4:
    at most 8 R / 3, the larger of the two, and the same for y.  The sample is continuous from cell to cell, and across an edge or
    a corner if the seam rule is right -- which is what this test is for.  Along the great arc between the two directions,
    |d out| <= (8 R / 3) (|dx| + |dy|) <= (8 R / 3) sqrt(2) |d(x, y)|.  On a face (x, y) = N / 2 (u, v) + const with (u, v) the
    gnomonic projection, whose stretch is at most 1 + u^2 + v^2 <= 3: |d(x, y)| <= 3 N / 2 d theta.  The product is
    4 sqrt(2) N R theta."""
    rng = np.random.default_rng(4)
    tex = rng.standard_normal((6, N, N, 3), dtype=np.float32)
    R = float(tex.max() - tex.min())
    worst = 0.0
    for theta in (1e-2 / N, 1e-4 / N):
        # within theta / 2 of an edge (of two edges: a corner) in face coordinates, so at most that angle away from it
        base = _near_seams(rng, 3000, N, reach=0.25 * theta * N)[0, 0, :, 0]
        base /= np.linalg.norm(base, axis=-1, keepdims=True)
        axis = np.cross(base, rng.standard_normal(base.shape))
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        side = np.cross(axis, base)                                       # unit, orthogonal to base
        p = np.cos(theta) * base + np.sin(theta) * side
        m = np.cos(theta) * base - np.sin(theta) * side
        sp, sm = ref.stage(_as_slots(p), N, None, "linear", np.float64), ref.stage(_as_slots(m), N, None, "linear", np.float64)
        crossed = sp["face"] != sm["face"]
        assert crossed.sum() > 300, (N, theta, int(crossed.sum()))
        assert ((sp["miss"] >= 0) | (sm["miss"] >= 0)).sum() > 300
        op, om = ref.forward64(_as_slots(p), tex), ref.forward64(_as_slots(m), tex)
        bound = 4 * np.sqrt(2) * N * R * (2 * theta)
        d = float(np.abs(op - om).max())
        worst = max(worst, d / bound)
        assert d <= bound + 1e-12, (N, theta, d, bound)
    print(N, "worst |difference| / bound", worst)


def _fd_set(rng, N, B):
    """(B,H,W,L,3) float64 directions -- random ones, ones near edges and ones near corners -- kept 0.1 texel away from every
    floor jump (fx, fy in [0.1, 0.9]) and from every face switch (x, y 0.1 inside [-0.5, N - 0.5])."""
    cand = np.concatenate([_dirs(rng, 4000, np.float64), _near_seams(rng, 4000, N)], 2)[0, 0, :, 0]
    st = ref.stage(_as_slots(cand), N, None, "linear", np.float64)
    ok = np.ones(cand.shape[0], bool)
    for f, x in ((st["fx"], st["x"]), (st["fy"], st["y"])):
        f, x = f[0, 0, :, 0], x[0, 0, :, 0]
        ok &= (f >= 0.1) & (f <= 0.9) & (x >= -0.4) & (x <= N - 0.6)
    keep = cand[ok]
    n = (keep.shape[0] // (B * 6)) * B * 6
    return keep[:n].reshape(B, 2, -1, 3, 3)


@pytest.mark.parametrize("per_view", (False, True))
@pytest.mark.parametrize("N", (1, 4))
def test_grads64_against_central_differences(N, per_view):
    rng = np.random.default_rng(5)
    B, C = 2, 2
    d = _fd_set(rng, N, B)
    shape = d.shape[:4]
    tex = rng.standard_normal(((B,) if per_view else ()) + (6, N, N, C))
    rl = rng.integers(-1, 3, shape).astype(np.int32)
    g = rng.standard_normal(shape + (C,))
    st = ref.stage(d, N, rl, "linear", np.float64)
    live = ~st["empty"]
    assert ((st["miss"] >= 0) & live).sum() > 50, "corner samples (three taps)"
    if N == 1:                                                            # x, y in [-0.5, 0.5]: every sample is a corner sample
        assert ((st["miss"] >= 0) == live).all()
    else:
        assert (st["seam"].any(-1) & (st["miss"] < 0) & live).sum() > 50, "edge samples"
        assert (~st["seam"].any(-1) & live).sum() > 50, "interior samples"
    dtex, ddir = ref.grads64(d, tex, rl, "linear", g, stage_dtype=np.float64)

    def slot_loss(d_, tex_):
        return (ref.forward64(d_, tex_, rl) * g).sum(-1)
    h = 1e-4
    fd = np.zeros_like(tex)
    for k in range(tex.size):
        p, m = tex.copy(), tex.copy()
        p.reshape(-1)[k] += h
        m.reshape(-1)[k] -= h
        fd.reshape(-1)[k] = (slot_loss(d, p).sum() - slot_loss(d, m).sum()) / (2 * h)
    assert np.abs(dtex).max() > 0 and np.abs(fd - dtex).max() <= 1e-8 * np.abs(dtex).max()
    # a slot's sample depends on its own direction alone: all slots are perturbed at once, one component at a time.
    # |d(x, y)| <= 3 N / 2 |d dir| / |dir|: with |dir| >= e^-2 a step of 1e-6 moves a sample by < 1e-4 texels, inside the margin
    h = 1e-6
    fd = np.zeros_like(d)
    for k in range(3):
        p, m = d.copy(), d.copy()
        p[..., k] += h
        m[..., k] -= h
        fd[..., k] = (slot_loss(p, tex) - slot_loss(m, tex)) / (2 * h)
    assert np.abs(ddir).max() > 0 and np.abs(fd - ddir).max() <= 1e-6 * np.abs(ddir).max()
    assert (ddir[rl < 0] == 0).all()
    # scale invariance: the gradient is orthogonal to the direction
    dot = (ddir * d).sum(-1)
    assert np.abs(dot).max() <= 1e-12 * (np.abs(ddir) * np.abs(d)).sum(-1).max()
    # nearest: weight one on the one texel, nothing to the direction
    dtex_n, ddir_n = ref.grads64(d, tex, rl, "nearest", g, stage_dtype=np.float64)
    assert (ddir_n == 0).all()
    fd = np.zeros_like(tex)
    base = ref.forward64(d, tex, rl, "nearest")
    for k in range(tex.size):
        p = tex.copy()
        p.reshape(-1)[k] += 1.0
        fd.reshape(-1)[k] = float(((ref.forward64(d, p, rl, "nearest") - base) * g).sum())
    assert np.abs(fd - dtex_n).max() <= 1e-12 * max(np.abs(dtex_n).max(), 1.0)


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
@pytest.mark.parametrize("per_view", (False, True))
@pytest.mark.parametrize("N", (1, 3))
def test_dtex_sums_to_the_upstream_gradient_and_ddir_is_orthogonal(N, per_view, filter_mode):
    """The weights of a sample add to one (at a corner after the renormalisation): dL/dtex sums, per channel, to g summed
    over the non-empty slots; and the float32-stage gradient of the direction is orthogonal to it."""
    rng = np.random.default_rng(6)
    B, C = 2, 4
    d = np.concatenate([_dirs(rng, 2400), _near_seams(rng, 600, N).astype(np.float32)], 2).reshape(B, 10, 30, 6, 3)
    rl = rng.integers(-1, 5, d.shape[:4]).astype(np.int32)
    tex = rng.standard_normal(((B,) if per_view else ()) + (6, N, N, C), dtype=np.float32)
    g = rng.standard_normal(d.shape[:4] + (C,))
    dtex, ddir = ref.grads64(d, tex, rl, filter_mode, g)
    live = ~ref.empty(d, rl)
    assert np.array_equal(live, rl >= 0)
    if per_view:
        for b in range(B):
            assert np.allclose(dtex[b].sum((0, 1, 2)), g[b][live[b]].sum(0), rtol=0, atol=1e-9)
    else:
        assert np.allclose(dtex.sum((0, 1, 2)), g[live].sum(0), rtol=0, atol=1e-9)
    dot = (ddir * d.astype(np.float64)).sum(-1)
    assert np.abs(dot).max() <= 1e-12 * max((np.abs(ddir) * np.abs(d)).sum(-1).max(), 1e-30)
    assert (filter_mode == "nearest") == (not ddir.any())


@pytest.mark.parametrize("filter_mode", ref.FILTERS)
def test_empty_slots(filter_mode):
    rng = np.random.default_rng(7)
    N, C = 4, 2
    d = _dirs(rng, 128).reshape(1, 8, 8, 2, 3)
    rl = np.zeros(d.shape[:4], np.int32)
    bad = np.zeros(d.shape[:4], bool)
    fd, frl, fbad = d.reshape(-1, 3), rl.reshape(-1), bad.reshape(-1)
    cases = ((np.nan, 1, 1), (1, np.nan, 1), (1, 1, np.nan), (np.inf, 1, 1), (1, -np.inf, 1), (1, 1, np.inf), (0, 0, 0),
             (-0.0, 0.0, -0.0), (-0.0, -0.0, -0.0), (np.inf, np.inf, np.inf))
    for k, c in enumerate(cases):
        fd[3 * k] = c
        fbad[3 * k] = True
    for k in (40, 41, 77):
        frl[k] = -1 - k                                                   # (a good direction: empty by the id alone)
        fbad[k] = True
    fd[50], fd[51], fd[52] = (-0.0, 2.0, 0.0), (0.0, -0.0, -1e-30), (1e30, -0.0, 0.0)      # zeros beside a live component: not empty
    assert np.array_equal(ref.empty(d, rl), bad)
    assert np.array_equal(ref.empty(d, None), bad & (rl >= 0))
    tex = rng.standard_normal((6, N, N, C), dtype=np.float32) + 10
    out = ref.forward32(d, tex, rl, filter_mode)
    assert (out[bad] == 0).all() and (out[~bad] != 0).all() and np.isfinite(out).all()
    g = np.ones(d.shape[:4] + (C,))
    dtex, ddir = ref.grads64(d, tex, rl, filter_mode, g)
    assert (ddir[bad] == 0).all() and np.isfinite(ddir).all()
    assert np.allclose(dtex.sum((0, 1, 2)), (~bad).sum(), rtol=0, atol=1e-9)
    assert ref.stage(d, N, rl, filter_mode)["face"].reshape(-1)[[50, 51, 52]].tolist() == [2, 5, 0]


def test_ties_pick_the_documented_face():
    """x before y before z: |x| == |y| picks x, |y| == |z| (above |x|) picks y, all three equal picks x; the sign is the major
    component's own."""
    cases = {(1, 1, 0): 0, (-1, 1, 0): 1, (1, -1, 0.5): 0, (0.5, 1, 1): 2, (0.5, -1, 1): 3, (0, 1, -1): 2, (1, 1, 1): 0,
             (-1, -1, -1): 1, (-1, 1, 1): 1, (1, 0.5, 1): 0, (-1, 0.5, -1): 1, (0.5, 0.5, 1): 4, (0.5, 0.5, -1): 5, (0, 0, -3): 5}
    d = _as_slots(np.array(list(cases), np.float32))
    for filter_mode in ref.FILTERS:
        st = ref.stage(d, 4, None, filter_mode)
        assert st["face"].reshape(-1).tolist() == list(cases.values())
    # nearest on a tie: the clamp keeps the texel on the chosen face's border
    st = ref.stage(d, 4, None, "nearest")
    assert (st["idx"][..., 0] // 16 == st["face"]).all()


def test_distinct_texels_per_tile():
    rng = np.random.default_rng(8)
    d = rng.standard_normal((1, 32, 32, 2, 3)).astype(np.float32)
    d[:, :, :, 1] = (1.0, 1.0, 1.0)                                       # layer 1: every pixel on one cube corner
    assert ref.distinct_texels_per_tile(d[:, :, :, 1:], 8, None, "linear") == 3
    assert ref.distinct_texels_per_tile(d[:, :, :, 1:], 8, None, "nearest") == 1
    assert ref.distinct_texels_per_tile(d[:, :, :, :1], 1024, None, "linear") > 900
    assert ref.distinct_texels_per_tile(d, 8, np.full((1, 32, 32, 2), -1, np.int32)) == 0


@pytest.mark.parametrize("N", ref.INST_NS)
def test_instantiation_inputs_are_what_they_are_for(N):
    """The inputs of test_gpu_texture_cube.py's test_every_instantiation_once: every tile has live and empty slots in both
    layers; a seam-crossing sample across each of the 24 (face, border) pairs; corner samples (a missing tap)."""
    d, rl = ref.instantiation_case(N)
    st = ref.stage(d, N, rl, "linear")
    live = ~st["empty"]
    assert ref2d.tiles_have_live_and_empty(st["empty"])
    bad = ~np.isfinite(d).all(-1)
    assert bad.sum() == 6 and np.array_equal(st["empty"], (rl < 0) | bad)
    borders = (st["i0"] == -1, st["i0"] == N - 1, st["j0"] == -1, st["j0"] == N - 1)
    for f in range(6):
        for k, b in enumerate(borders):
            assert (live & (st["face"] == f) & b & st["seam"].any(-1)).any(), (N, "face", f, "border", k)
    corners = int((live & (st["miss"] >= 0)).sum())
    print("N", N, "seam samples", int((live & st["seam"].any(-1)).sum()), "corner samples", corners)
    assert corners >= 8 and set(np.unique(st["miss"][live]).tolist()) == {-1, 0, 1, 2, 3}
