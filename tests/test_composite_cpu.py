"""The restatement of Renderer.composite's contract (tests/composite_ref.py) against independent routes, on the CPU: grads64
against float64 torch autograd at the same stop and against central differences, forward32 against the torch line users
write, forward32 fed interpolate_ref's colours against layer_composite_ref (LayeredRenderer.render's restatement), and the
conditions the GPU tests' inputs must meet, so that those tests cannot run hollow."""
import os
import re

import numpy as np
import pytest
import torch

import composite_ref as ref
import interpolate_ref as iref
import layer_composite_ref as lref
import rasterize_ref as rref
from util import ROOT, rel_linf, table_capacity


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _forward64(values, a, blend, background):
    """The blend over the given slots in float64 torch (differentiable in values and the per-slot a) -> (out, acc)."""
    B, H, W, L, C = values.shape
    T = torch.ones((B, H, W), dtype=torch.float64)
    O = torch.zeros((B, H, W, C), dtype=torch.float64)
    for l in range(L):
        m = blend[..., l]
        al = torch.where(m, a[..., l], torch.zeros((), dtype=torch.float64))
        O = O + torch.where(m[..., None], values[..., l, :], torch.zeros((), dtype=torch.float64)) * (al * T)[..., None]
        T = T * (1 - al)
    if background is not None:
        O = O + T[..., None] * background
    return O, 1 - T


def _autograd64(c, use_g=True, use_gA=True):
    """float64 torch autograd of the forward at the case's float32 stop index and empty mask -> (dvalues, dalpha)."""
    alpha, rl = c["alpha"], c["render_layers"]
    blend = torch.from_numpy(ref.blended(alpha, rl, c["n_contrib"]))
    v = torch.tensor(np.where(blend.numpy()[..., None], c["values"], 0).astype(np.float64), requires_grad=True)
    al = torch.tensor(alpha.astype(np.float64), requires_grad=True)
    a = al[torch.from_numpy(np.clip(rl, 0, alpha.shape[0] - 1).astype(np.int64))] if alpha.ndim == 1 else al
    a = torch.where(blend, a, torch.zeros((), dtype=torch.float64))           # (NaNs of unblended slots stay out of the graph)
    bg = None if c["background"] is None else torch.from_numpy(c["background"].astype(np.float64))
    out, acc = _forward64(v, a, blend, bg)
    loss = torch.zeros((), dtype=torch.float64)
    if use_g:
        loss = loss + (out * torch.from_numpy(c["g"].astype(np.float64))).sum()
    if use_gA:
        loss = loss + (acc * torch.from_numpy(c["gA"].astype(np.float64))).sum()
    loss.backward()
    return (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.numpy()), al.grad.numpy()


GRID = [(L, C, pf) for L in ref.LS for C, pf in (((3, False), (4, True)) if L % 2 else ((16, False), (1, True)))]


@pytest.mark.parametrize("L,C,per_face", GRID)
def test_grads64_against_float64_autograd(L, C, per_face):
    """The back pass (no division) against autograd of the float64 forward at the same stop.  Both are float64 evaluations of
    one polynomial of degree <= L in the alphas: 1e-12 relative leaves four digits over the eps 2.2e-16 times the L * C terms."""
    c = ref.case(L, C, per_face)
    for use_g, use_gA in ((True, True), (True, False), (False, True)):
        wv, wa = ref.grads64(c["values"], c["alpha"], c["render_layers"], c["background"], c["n_contrib"],
                             c["g"] if use_g else None, c["gA"] if use_gA else None)
        tv, ta = _autograd64(c, use_g, use_gA)
        ev, ea = rel_linf(wv, tv), rel_linf(wa, ta)
        print(L, C, per_face, use_g, use_gA, "dvalues", ev, "dalpha", ea)
        assert np.abs(ta).max() > 0 and (np.abs(tv).max() > 0) == use_g
        assert ev <= 1e-12 and ea <= 1e-12
        assert not wv[~c["blend"]].any()
        if not per_face:
            assert not wa[~c["blend"]].any()


@pytest.mark.parametrize("per_face", [False, True])
def test_grads64_against_central_differences(per_face):
    """Central differences of a float64 forward that decides its own stop, along random directions and single elements, on
    inputs with no pixel within a factor 2 of T_EPS at any slot (a step of 1e-6 then moves no stop, an alpha of exactly 1 included: T = 1e-6 T_l stays below T_EPS).  The loss is a polynomial
    of degree <= L = 5 in the alphas of size O(1): the h^2 term is below 1e-11, rounding (eps |loss| / h, |loss| ~ 1e3) near 1e-7 absolute against gradients of size 1e2; the bar is 1e-6 relative."""
    c = dict(ref.case(5, 3, per_face))
    a, empty = ref.slots(c["alpha"], c["render_layers"], np.float64)
    # prefix transmittances of the float64 walk; pixels that come near the stop are emptied
    T = np.cumprod(np.where(empty, 1.0, 1 - a), -1)
    near = ((T > ref.T_EPS / 2) & (T < ref.T_EPS * 2)).any(-1)
    rl = c["render_layers"].copy()
    rl[near] = -1
    out, fT, n, blend = ref.forward32(c["values"], c["alpha"], rl, c["background"], full=True)
    assert near.mean() < 0.2 and (fT < ref.T_EPS).mean() > 0.05 and ((n > 0) & (fT >= ref.T_EPS)).mean() > 0.05
    wv, wa = ref.grads64(c["values"], c["alpha"], rl, c["background"], n, c["g"], c["gA"])
    g, gA, bg = (c[k].astype(np.float64) for k in ("g", "gA", "background"))

    def loss(values, alpha):
        al, em = ref.slots(alpha, rl, np.float64)
        Tn = np.ones(fT.shape)
        O = np.zeros(out.shape)
        done = np.zeros(fT.shape, bool)
        for l in range(al.shape[-1]):
            act = ~em[..., l] & ~done
            x = np.where(act, al[..., l], 0.0)
            O = O + np.where(act[..., None], values[..., l, :], 0.0) * (x * Tn)[..., None]
            Tn = Tn * (1 - x)
            done |= act & (Tn < ref.T_EPS)
        return float((g * (O + Tn[..., None] * bg)).sum() + (gA * (1 - Tn)).sum())

    v0, a0 = c["values"].astype(np.float64), c["alpha"].astype(np.float64)
    rng = np.random.default_rng(3)
    h = 1e-6
    scale = max(np.abs(wv).max(), np.abs(wa).max())
    for k in range(3):
        dv, da = rng.standard_normal(v0.shape), rng.standard_normal(a0.shape)
        fd = (loss(v0 + h * dv, a0 + h * da) - loss(v0 - h * dv, a0 - h * da)) / (2 * h)
        an = (wv * dv).sum() + (wa * da).sum()
        print("direction", k, fd, an)
        assert abs(fd - an) <= 1e-6 * max(abs(an), scale)
    cand = np.argwhere(blend) if not per_face else np.argwhere(wa != 0)
    for idx in cand[rng.choice(len(cand), 12, replace=False)]:
        da = np.zeros(a0.shape)
        da[tuple(idx)] = 1.0
        fd = (loss(v0, a0 + h * da) - loss(v0, a0 - h * da)) / (2 * h)
        assert abs(fd - wa[tuple(idx)]) <= 1e-6 * scale, (idx, fd, wa[tuple(idx)])
    for idx in np.argwhere(blend)[rng.choice(int(blend.sum()), 12, replace=False)]:
        dv = np.zeros(v0.shape)
        dv[tuple(idx) + (1,)] = 1.0
        fd = (loss(v0 + h * dv, a0) - loss(v0 - h * dv, a0)) / (2 * h)
        assert abs(fd - wv[tuple(idx) + (1,)]) <= 1e-6 * scale, (idx, fd)


@pytest.mark.parametrize("per_face", [False, True])
@pytest.mark.parametrize("bg", [False, True])
def test_forward32_against_the_one_liner(per_face, bg):
    """Opacities <= 0.85 and L = 4: T stays above 0.15^4 = 5e-4, no pixel stops, and the op computes what the torch line does.
    Two float32 routes (the weights as a T against a running product shifted): a few ulp of values of size O(1) times L."""
    c = ref.case(4, 3, per_face, bg=bg)
    alpha = np.minimum(c["alpha"], np.float32(0.85))
    out, T, n = ref.forward32(c["values"], alpha, c["render_layers"], c["background"])
    assert (T >= ref.T_EPS).all() and (T < 1).any()
    t = lambda x: None if x is None else torch.from_numpy(x)
    o1, a1 = ref.one_liner(t(c["values"]), t(alpha), t(c["render_layers"]), t(c["background"]))
    assert np.abs(out - o1.numpy()).max() <= 1e-5 and np.abs((np.float32(1) - T) - a1.numpy()).max() <= 1e-6
    assert np.abs(out).max() > 1


_XCHECK = {}


def xcheck_inputs(name, L):
    """rasterize_ref's hits on a scene and composite_ref.render_tables -> what both restatements take."""
    if (name, L) not in _XCHECK:
        s = rref.scene(name)
        ras = rref.rasterize32(s["W"], s["H"], s["verts"], s["faces"], None, s["verts_ndc"], s["verts_image"], s["ray_o"], s["ray_d"], L)
        P, F, B = s["verts"].shape[0], s["faces"].shape[0], s["verts_ndc"].shape[0]
        _XCHECK[(name, L)] = dict(s=s, ras=ras, **ref.render_tables(P, F, B, L))
    return _XCHECK[(name, L)]


@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("name", ["soup", "lattice", "degenerate"])
def test_composite_of_interpolated_colours_is_render(name, L):
    """composite(interpolate(verts_color), faces_opacity) is LayeredRenderer.render's blend: final_T bit-equal, n_contrib equal,
    colour within 1e-6 absolute (colours in [0, 1]; one ulp from (c a) T against c (a T)), no pixel excused."""
    x = xcheck_inputs(name, L)
    s, ras = x["s"], x["ras"]
    want = lref.forward32(ras["layers"], s["verts"], s["faces"], x["color"], x["opacity"], x["intense"], s["verts_ndc"],
                          x["background"], s["ray_o"], s["ray_d"])
    values = iref.forward32(ras["layers"], ras["bary"], x["color"], s["faces"])
    out, T, n = ref.forward32(values, x["opacity"], ras["layers"], x["background"])
    assert (n > 0).mean() > 0.2 and (T < ref.T_EPS).sum() > 4, ((n > 0).mean(), (T < ref.T_EPS).mean())
    assert np.array_equal(_bits(T), _bits(want["final_T"]))
    assert np.array_equal(n, want["n_contrib"])
    err = float(np.abs(out - want["color"]).max())
    print(name, L, "colour", err)
    assert err <= 1e-6


@pytest.mark.parametrize("L", ref.LS)
def test_gpu_cases_meet_their_conditions(L):
    for per_face in (False, True):
        ref.check_case(ref.case(L, 3, per_face))
    c = ref.case(L, 3, False, layers=False)
    assert c["render_layers"] is None and c["blend"][..., 0].all()


def test_layer_counts_straddle_the_kernels_chunk():
    """The kernels take the slots in chunks of CP_LCH: the tested L hold k chunks and k chunks + 1 for k = 1, 2, 3, next to the
    issue's list."""
    src = open(os.path.join(ROOT, "dmesh2_renderer_amd", "csrc", "dm2_composite.hip")).read()
    chunk = int(re.search(r"constexpr int CP_LCH = (\d+);", src).group(1))
    assert chunk == ref.CHUNK
    assert {k * chunk + d for k in (1, 2, 3) for d in (0, 1)} <= set(ref.LS) and {1, 2, 4, 5, 8, 9, 17, 33} <= set(ref.LS)
    assert set(ref.CS) == {1, 2, 3, 4, 7, 16, 33}


@pytest.mark.parametrize("name", sorted(ref.CROWDED))
def test_crowded_cases_meet_their_conditions(name):
    lo, hi = ref.check_crowded(name, ref.crowded(name), table_capacity())
    print(name, "distinct blended faces per tile", lo, hi)


def test_distinct_blended_per_tile():
    rl = np.zeros((1, 32, 32, 2), np.int32)
    rl[0, :16, :16, 0] = np.arange(256).reshape(16, 16)
    rl[0, :16, :16, 1] = 999
    blend = np.ones(rl.shape, bool)
    blend[0, :16, :16, 1] = False
    assert ref.distinct_blended_per_tile(rl, blend) == (1, 256)


def test_empty_and_behind_the_stop_are_not_looked_at():
    """NaN and inf in the values and alphas of empty slots and of slots behind the stop change no bit of forward32 or grads64;
    a blended slot with alpha 0 still adds (inf * 0 = NaN reaches the output)."""
    c = ref.case(5, 3, False)
    v, a = c["values"].copy(), c["alpha"].copy()
    dead = ~c["blend"]
    v[dead] = np.where(np.arange(dead.sum())[:, None] % 2 == 0, np.nan, np.inf)
    a[dead] = np.nan
    out, T, n = ref.forward32(v, a, c["render_layers"], c["background"])
    assert np.array_equal(_bits(out), _bits(c["out"])) and np.array_equal(_bits(T), _bits(c["final_T"])) and np.array_equal(n, c["n_contrib"])
    g0 = ref.grads64(c["values"], c["alpha"], c["render_layers"], c["background"], n, c["g"], c["gA"])
    g1 = ref.grads64(v, a, c["render_layers"], c["background"], n, c["g"], c["gA"])
    assert np.array_equal(g0[0], g1[0]) and np.array_equal(g0[1], g1[1])
    zero = c["blend"] & (ref.slots(c["alpha"], c["render_layers"])[0] == 0)
    v2 = c["values"].copy()
    v2[zero] = np.inf
    out2 = ref.forward32(v2, c["alpha"], c["render_layers"], c["background"])[0]
    assert zero.any() and np.isnan(out2[zero.any(-1)]).all()
