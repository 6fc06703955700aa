"""Restatement of Renderer.composite's contract (include/dm2_hip.h: dm2_composite / dm2_composite_backward) in numpy.

values (B,H,W,L,C); alpha (B,H,W,L) per slot or (F,) per face (gathered as alpha[render_layers]); render_layers (B,H,W,L) or
None; background (C,) or None.  A slot is empty when its id is negative or, with a per-face alpha, outside [0, F).  Per pixel,
from T = 1, O = 0, n = 0, over the slots in order: an empty slot is skipped; otherwise w = a * T, O_c = O_c + values[l,c] * w,
T = T * (1 - a), n = l + 1, and the walk stops once T < T_EPS.  out = O + T * background, acc = 1 - T.

* ``forward32`` -- float32, vectorised numpy, in the device's operation order (numpy float32 arithmetic is IEEE and
  uncontracted, like the kernels built with -ffp-contract=off): what the kernel must match bit for bit.
* ``grads64`` -- the contract's backward (T_l front to back, then the back pass R <- a S + (1 - a) R from R = K) in float64,
  given the float32 forward's stop index.
* ``one_liner`` -- the torch expression users write without the op (no stop).
* ``case`` / ``crowded`` -- the hand-built inputs of the CPU and GPU tests, and the conditions they must meet.
"""
import numpy as np
import torch

T_EPS = np.float32(0.0001)
f32 = np.float32
TILE = 16                   # the per-face backward's tile: one block, one face table


def slots(alpha, render_layers, dtype=f32):
    """-> (a (B,H,W,L) ``dtype``: each slot's alpha, 0 in empty slots; empty (B,H,W,L) bool)."""
    alpha = np.asarray(alpha)
    if alpha.ndim == 1:
        rl = np.asarray(render_layers)
        F = alpha.shape[0]
        empty = (rl < 0) | (rl >= F)
        a = alpha[np.where(empty, 0, rl)] if F else np.zeros(rl.shape, alpha.dtype)
    else:
        empty = np.zeros(alpha.shape, bool) if render_layers is None else np.asarray(render_layers) < 0
        a = alpha
    return np.where(empty, 0, a).astype(dtype), empty


def forward32(values, alpha, render_layers=None, background=None, full=False):
    """-> out (B,H,W,C), final_T (B,H,W), n_contrib (B,H,W) int32 [, blend (B,H,W,L) bool with ``full``]."""
    values = np.asarray(values, dtype=f32)
    a, empty = slots(alpha, render_layers)
    B, H, W, L, C = values.shape
    T = np.ones((B, H, W), f32)
    O = np.zeros((B, H, W, C), f32)
    n = np.zeros((B, H, W), np.int32)
    done = np.zeros((B, H, W), bool)
    blend = np.zeros((B, H, W, L), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            act = ~empty[..., l] & ~done
            al = np.where(act, a[..., l], f32(0))
            w = (al * T).astype(f32)
            v = np.where(act[..., None], values[..., l, :], f32(0))
            O = np.where(act[..., None], O + (v * w[..., None]).astype(f32), O).astype(f32)
            T = np.where(act, T * (f32(1) - al), T).astype(f32)
            n = np.where(act, l + 1, n).astype(np.int32)
            done = done | (act & (T < T_EPS))
            blend[..., l] = act
        out = O if background is None else (O + (T[..., None] * np.asarray(background, dtype=f32)).astype(f32)).astype(f32)
    return (out, T, n, blend) if full else (out, T, n)


def blended(alpha, render_layers, n_contrib):
    """(B,H,W,L) bool: not empty and in front of the stop."""
    _, empty = slots(alpha, render_layers)
    return ~empty & (np.arange(empty.shape[-1]) < np.asarray(n_contrib)[..., None])


def grads64(values, alpha, render_layers, background, n_contrib, g=None, gA=None):
    """(dL/dvalues (B,H,W,L,C), dL/dalpha of alpha's shape) in float64 for upstream g (B,H,W,C) and gA (B,H,W), either may be
    None (zero): the contract's backward at the float32 forward's stop index ``n_contrib`` and empty mask."""
    values = np.asarray(values)
    B, H, W, L, C = values.shape
    blend = blended(alpha, render_layers, n_contrib)
    a = np.where(blend, slots(alpha, render_layers, np.float64)[0], 0.0)
    v = np.where(blend[..., None], values, 0).astype(np.float64)
    g = np.zeros((B, H, W, C)) if g is None else np.asarray(g, dtype=np.float64)
    gA = np.zeros((B, H, W)) if gA is None else np.asarray(gA, dtype=np.float64)
    Tl = np.zeros((B, H, W, L))
    T = np.ones((B, H, W))
    for l in range(L):
        Tl[..., l] = T
        T = np.where(blend[..., l], T * (1 - a[..., l]), T)
    dvalues = np.where(blend[..., None], (a * Tl)[..., None] * g[..., None, :], 0.0)
    S = (g[..., None, :] * v).sum(-1)
    R = -gA if background is None else (g * np.asarray(background, dtype=np.float64)).sum(-1) - gA
    da = np.zeros((B, H, W, L))
    for l in range(L - 1, -1, -1):
        b = blend[..., l]
        da[..., l] = np.where(b, Tl[..., l] * (S[..., l] - R), 0.0)
        R = np.where(b, a[..., l] * S[..., l] + (1 - a[..., l]) * R, R)
    if np.asarray(alpha).ndim == 1:
        F = np.asarray(alpha).shape[0]
        da = np.bincount(np.asarray(render_layers)[blend].astype(np.int64), weights=da[blend], minlength=F)
    return dvalues, da


def one_liner(values, alpha, render_layers=None, background=None):
    """What users write without the op, in torch (differentiable; no T < T_EPS stop) -> (out (B,H,W,C), acc (B,H,W))."""
    if alpha.dim() == 1:
        ok = (render_layers >= 0) & (render_layers < alpha.shape[0])
        a = torch.where(ok, alpha[render_layers.clamp(0, alpha.shape[0] - 1).long()], torch.zeros_like(values[..., 0]))
    else:
        a = alpha if render_layers is None else torch.where(render_layers >= 0, alpha, torch.zeros_like(alpha))
    trans = torch.cumprod(1 - a, -1)
    front = torch.cat([torch.ones_like(trans[..., :1]), trans[..., :-1]], -1)
    out = (values * (a * front)[..., None]).sum(-2)
    if background is not None:
        out = out + trans[..., -1:] * background
    return out, 1 - trans[..., -1]


def distinct_blended_per_tile(render_layers, blend, tile=TILE):
    """-> (smallest, largest) number of distinct blended faces over the tile x tile pixel tiles of every view: what a block of
    the per-face backward asks of its face table (dm2_face_table.h)."""
    rl = np.asarray(render_layers)
    B, H, W, _ = rl.shape
    counts = []
    for b in range(B):
        for y in range(0, H, tile):
            for x in range(0, W, tile):
                counts.append(len(np.unique(rl[b, y:y + tile, x:x + tile][blend[b, y:y + tile, x:x + tile]])))
    return min(counts), max(counts)


# ---- the tests' inputs -----------------------------------------------------------------------------------------------------
CHUNK = 8                                         # CP_LCH of dm2_composite.hip: the slots go through the kernels in chunks
LS = (1, 2, 4, 5, 8, 9, 16, 17, 24, 25, 33)       # the issue's list plus k * CHUNK and k * CHUNK + 1
CS = (1, 2, 3, 4, 7, 16, 33)
SHAPE = (2, 37, 50)                               # partial tiles and a partial last block
F_CASE = 211


def _alphas(rng, shape, L):
    """alpha in [0, 1], about 10 % exactly 1 and 10 % exactly 0.  L > 16: uniform in [0, 16 / L] and a share of 1 / L at exactly
    1, so that neither the opaque slots nor the product end (nearly) every list in its first third."""
    hi, ones = min(1.0, 16.0 / L), min(0.1, 1.0 / L)
    a = rng.uniform(0.0, hi, shape).astype(f32)
    m = rng.uniform(size=shape)
    a[m < ones] = 1.0
    a[m > 0.9] = 0.0
    return a


_CASES = {}


def case(L, C, per_face, layers=True, bg=True, keep=True):
    """dict(values, alpha, render_layers or None, background or None, g, gA, out, final_T, n_contrib, blend): hand-built random
    inputs at SHAPE and their float32 forward.  20 % of the ids are -1, 4 % of the pixels have every slot empty; with a
    per-face alpha 3 % of the ids lie beyond F as well.  (Cached unless ``keep`` is
    False: leave the arrays unchanged.)"""
    key = (L, C, per_face, layers, bg)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * L + 10 * C + per_face)
        shape = SHAPE + (L,)
        rl = rng.integers(0, F_CASE, shape).astype(np.int32)
        m = rng.uniform(size=shape)
        rl[m < 0.2] = -1
        if per_face:
            rl[(m >= 0.2) & (m < 0.23)] = F_CASE + rng.integers(0, 5)
        rl[rng.uniform(size=SHAPE) < 0.04] = -1
        alpha = _alphas(rng, (F_CASE,) if per_face else shape, L)
        c = dict(values=rng.standard_normal(shape + (C,), dtype=f32), alpha=alpha,
                 render_layers=rl if (layers or per_face) else None,
                 background=rng.uniform(0, 1, C).astype(f32) if bg else None,
                 g=rng.standard_normal(SHAPE + (C,), dtype=f32), gA=rng.standard_normal(SHAPE, dtype=f32))
        c["out"], c["final_T"], c["n_contrib"], c["blend"] = forward32(c["values"], alpha, c["render_layers"], c["background"], full=True)
        if not keep:
            return c
        _CASES[key] = c
    return _CASES[key]


def check_case(c):
    """What a case must exercise, on the restatement alone: empty slots and wholly empty pixels (with ids), blended slots with
    alpha exactly 0 and exactly 1, and -- from three slots on -- each third of the list holding the last blend of at least 5 %
    of the pixels while at least 5 % never stop."""
    a, empty = slots(c["alpha"], c["render_layers"])
    blend, n, T = c["blend"], c["n_contrib"], c["final_T"]
    L = blend.shape[-1]
    if c["render_layers"] is not None:
        assert 0.15 < empty.mean() < 0.35 and (n == 0).mean() > 0.02, (empty.mean(), (n == 0).mean())
    assert (blend & (a == 0)).any() and (blend & (a == 1)).any()
    assert (blend == blended(c["alpha"], c["render_layers"], n)).all()
    if L >= 3:
        third = (np.maximum(n, 1) - 1) * 3 // L
        shares = [float(((n > 0) & (third == k)).mean()) for k in range(3)]
        never = float(((T >= T_EPS) & (n > 0)).mean())
        assert min(shares) >= 0.05 and never >= 0.05, (L, shares, never)
        assert ((T < T_EPS) & (n < L)).mean() >= 0.05, L                     # and stops with slots left behind them
    return a, empty


# The face table's overflow route (per-face alpha, B = 2, 48 x 64: twelve tiles a view), ids uniform in [0, F).  kind: "overflow"
# = every tile blends more distinct faces than the table has slots; "nearly_full" = fewer than it has slots but more than 0.8 of
# them, so that probe chains fail for some faces while free slots remain and both routes mix inside a tile; "fits" = well below.
CROWDED = {
    "overflow_L4": dict(F=4000, L=4, kind="overflow"),
    "overflow_L12": dict(F=4000, L=12, kind="overflow"),
    "nearly_full_L4": dict(F=600, L=4, kind="nearly_full"),
    "fits_L4": dict(F=300, L=4, kind="fits"),
}
_CROWDED = {}


def crowded(name, C=3):
    """A CROWDED case as ``case`` returns them: a face repeated within a pixel's list (every fifth row: slot 1 = slot 0), 1 % of
    the ids outside [0, F) on either side, opacities in [0.02, 1.6 / L] so that the lists do not end early, and of exactly 1
    and 0 (every 97th face each)."""
    if (name, C) not in _CROWDED:
        k = CROWDED[name]
        F, L = k["F"], k["L"]
        rng = np.random.default_rng(1)
        shape = (2, 48, 64, L)
        rl = rng.integers(0, F, shape).astype(np.int32)
        m = rng.uniform(size=shape)
        rl[m < 0.005] = -1
        rl[m > 0.995] = F + 2
        rl[:, ::5, :, 1] = rl[:, ::5, :, 0]
        alpha = rng.uniform(0.02, 1.6 / L, F).astype(f32)
        alpha[0::97] = 1.0
        alpha[50::97] = 0.0
        c = dict(values=rng.standard_normal(shape + (C,), dtype=f32), alpha=alpha, render_layers=rl,
                 background=rng.uniform(0, 1, C).astype(f32),
                 g=rng.standard_normal(shape[:3] + (C,), dtype=f32), gA=rng.standard_normal(shape[:3], dtype=f32))
        c["out"], c["final_T"], c["n_contrib"], c["blend"] = forward32(c["values"], alpha, rl, c["background"], full=True)
        _CROWDED[(name, C)] = c
    return _CROWDED[(name, C)]


def check_crowded(name, c, slots_):
    """The condition a crowded case relies on, on the restatement's counts alone -> (lo, hi)."""
    lo, hi = distinct_blended_per_tile(c["render_layers"], c["blend"])
    kind = CROWDED[name]["kind"]
    if kind == "overflow":
        assert lo > slots_, (name, lo, hi, slots_)
    elif kind == "nearly_full":
        assert hi <= slots_ and lo > 0.8 * slots_, (name, lo, hi, slots_)
    else:
        assert 0.4 * slots_ < lo and hi < 0.7 * slots_, (name, lo, hi, slots_)
    rl = c["render_layers"]
    F = c["alpha"].shape[0]
    assert (rl[:, ::5, :, 1] == rl[:, ::5, :, 0]).all() and (rl < 0).any() and (rl >= F).any()
    return lo, hi


def render_tables(P, F, B, L):
    """The tables of the cross-check with LayeredRenderer.render: random vertex colours in [0, 1] and opacities (every seventh
    face opaque, so that stacks end at the stop), faces_intense = 1 -> dict(color (P,3), opacity (F), intense (B,F), background)."""
    rng = np.random.default_rng(70 + L)
    op = rng.uniform(0.05, 0.95, F).astype(f32)
    op[::7] = 1.0
    return dict(color=rng.uniform(0, 1, (P, 3)).astype(f32), opacity=op, intense=np.ones((B, F), f32),
                background=np.array([0.2, 0.5, 0.9], f32))
