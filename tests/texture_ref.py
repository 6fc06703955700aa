"""Restatement of Renderer.texture's contract (include/dm2_hip.h: dm2_texture / dm2_texture_backward) in numpy.

uv (B,H,W,L,2) = (u, v), u along the texture's width; tex (Ht,Wt,C) shared by the views or (B,Ht,Wt,C); render_layers (B,H,W,L)
or None.  Texel centres at ((i + 0.5) / Wt, (j + 0.5) / Ht):

    x  = u * Wt - 0.5             y  = v * Ht - 0.5
    x0 = floor(x)   fx = x - x0   y0 = floor(y)   fy = y - y0

A slot is empty when its id is negative, or u / v is not finite, or |x| or |y| is not below 2^24: zeros out, no gradient,
nothing read through it.  Otherwise the four texels (i0 + p, j0 + q), addressed by wrap ((i % n) + n) % n or clamp
min(max(i, 0), n - 1), blend as a = t00 + fx (t10 - t00), b = t01 + fx (t11 - t01), out = a + fy (b - a); nearest takes
the texel (floor(x + 0.5), floor(y + 0.5)).
"""
import numpy as np

f32 = np.float32
FILTERS = ("linear", "nearest")
BOUNDARIES = ("wrap", "clamp")
RANGE = 2.0 ** 24


def _addr(i, n, boundary_mode):
    if boundary_mode == "wrap":
        return np.mod(i, n)                 # Python's %: non-negative for n > 0
    if boundary_mode == "clamp":
        return np.clip(i, 0, n - 1)
    raise ValueError(boundary_mode)


def stage(uv, Ht, Wt, render_layers, filter_mode, boundary_mode, dtype=f32):
    """The contract's first stage in ``dtype`` (float32: the contract itself) -> dict(empty (B,H,W,L) bool, x, y, fx, fy
    (B,H,W,L) ``dtype``, idx (B,H,W,L,4) int64 = j * Wt + i of t00, t10, t01, t11 (nearest: the one texel four times); zeros
    in empty slots)."""
    if filter_mode not in FILTERS:
        raise ValueError(filter_mode)
    uv = np.asarray(uv)
    u, v = uv[..., 0].astype(dtype), uv[..., 1].astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (u * dtype(Wt)).astype(dtype) - dtype(0.5)
        y = (v * dtype(Ht)).astype(dtype) - dtype(0.5)
        e = ~np.isfinite(u) | ~np.isfinite(v) | ~(np.abs(x) < RANGE) | ~(np.abs(y) < RANGE)
    if render_layers is not None:
        e = e | (np.asarray(render_layers) < 0)
    x, y = np.where(e, dtype(0), x).astype(dtype), np.where(e, dtype(0), y).astype(dtype)
    if filter_mode == "nearest":
        i = _addr(np.floor(x + dtype(0.5)).astype(np.int64), Wt, boundary_mode)
        j = _addr(np.floor(y + dtype(0.5)).astype(np.int64), Ht, boundary_mode)
        idx = np.repeat((j * Wt + i)[..., None], 4, -1)
        fx = fy = np.zeros(x.shape, dtype)
    else:
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0).astype(dtype), (y - y0).astype(dtype)
        i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
        a0, a1 = _addr(i0, Wt, boundary_mode), _addr(i0 + 1, Wt, boundary_mode)
        r0, r1 = _addr(j0, Ht, boundary_mode) * Wt, _addr(j0 + 1, Ht, boundary_mode) * Wt
        idx = np.stack([r0 + a0, r0 + a1, r1 + a0, r1 + a1], -1)
    idx = np.where(e[..., None], 0, idx)
    return dict(empty=e, x=x, y=y, fx=np.where(e, dtype(0), fx).astype(dtype), fy=np.where(e, dtype(0), fy).astype(dtype), idx=idx)


def empty(uv, Ht, Wt, render_layers=None):
    """(B,H,W,L) bool: the empty slots (the same for both filters and both boundary modes)."""
    return stage(uv, Ht, Wt, render_layers, "nearest", "clamp")["empty"]


def _flat_idx(idx, tex):
    """Rows of tex.reshape(-1, C) for the (B,H,W,L,4) texel indices (the view's own texture for a (B,Ht,Wt,C) one)."""
    if tex.ndim == 4:
        per = tex.shape[1] * tex.shape[2]
        return idx + (np.arange(idx.shape[0], dtype=np.int64) * per).reshape(-1, 1, 1, 1, 1)
    return idx


def blend(st, tex, filter_mode, dtype=f32):
    """The contract's second stage on ``stage``'s output: the texels gathered and blended in ``dtype``."""
    tex = np.asarray(tex)
    t = tex.astype(dtype, copy=False).reshape(-1, tex.shape[-1])[_flat_idx(st["idx"], tex)]      # (B,H,W,L,4,C)
    if filter_mode == "nearest":
        out = t[..., 0, :]
    else:
        fx, fy = st["fx"].astype(dtype)[..., None], st["fy"].astype(dtype)[..., None]
        t00, t10, t01, t11 = (t[..., k, :] for k in range(4))
        with np.errstate(invalid="ignore", over="ignore"):
            a = (t00 + (fx * (t10 - t00).astype(dtype)).astype(dtype)).astype(dtype)
            b = (t01 + (fx * (t11 - t01).astype(dtype)).astype(dtype)).astype(dtype)
            out = (a + (fy * (b - a).astype(dtype)).astype(dtype)).astype(dtype)
    return np.where(st["empty"][..., None], dtype(0), out).astype(dtype)


def forward(uv, tex, render_layers=None, filter_mode="linear", boundary_mode="wrap", dtype=f32):
    """The whole contract in ``dtype``: separate multiplies and adds, in the written order."""
    tex = np.asarray(tex)
    return blend(stage(uv, tex.shape[-3], tex.shape[-2], render_layers, filter_mode, boundary_mode, dtype), tex, filter_mode, dtype)


def forward32(uv, tex, render_layers=None, filter_mode="linear", boundary_mode="wrap"):
    return forward(uv, tex, render_layers, filter_mode, boundary_mode, f32)


def grads64(uv, tex, render_layers, filter_mode, boundary_mode, g):
    """(dL/dtex of tex's shape, dL/duv (B,H,W,L,2)) for upstream g (B,H,W,L,C): x, y, fx, fy and the addresses from the
    float32 stage, everything after in float64 (the derivative of the float32 function at its own fractions)."""
    tex = np.asarray(tex)
    Ht, Wt, C = tex.shape[-3:]
    st = stage(uv, Ht, Wt, render_layers, filter_mode, boundary_mode, f32)
    live = ~st["empty"]
    g = np.where(live[..., None], np.asarray(g).astype(np.float64), 0.0)
    rows = _flat_idx(st["idx"], tex)
    fx, fy = st["fx"].astype(np.float64), st["fy"].astype(np.float64)
    if filter_mode == "nearest":
        w = np.stack([np.ones_like(fx), np.zeros_like(fx), np.zeros_like(fx), np.zeros_like(fx)], -1)
        duv = np.zeros(fx.shape + (2,), np.float64)
    else:
        w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1)
        t = tex.reshape(-1, C)[rows].astype(np.float64)
        t00, t10, t01, t11 = (t[..., k, :] for k in range(4))
        d0, d1 = t10 - t00, t11 - t01
        a, b = t00 + fx[..., None] * d0, t01 + fx[..., None] * d1
        du = Wt * (g * (d0 + fy[..., None] * (d1 - d0))).sum(-1)
        dv = Ht * (g * (b - a)).sum(-1)
        duv = np.where(live[..., None], np.stack([du, dv], -1), 0.0)
    w = np.where(live[..., None], w, 0.0)
    n = tex.size // C
    dtex = np.zeros((n, C), np.float64)
    flat_rows = rows.reshape(-1)
    for c in range(C):
        dtex[:, c] = np.bincount(flat_rows, weights=(w * g[..., c, None]).reshape(-1), minlength=n)
    return dtex.reshape(tex.shape), duv


def distinct_texels_per_tile(uv, Ht, Wt, render_layers=None, filter_mode="linear", boundary_mode="wrap", tile=16, worst=min):
    """The smallest (``worst=max``: the largest) number of distinct texels the non-empty slots of one layer address, over the
    tile x tile pixel tiles of every view and over the layers."""
    st = stage(uv, Ht, Wt, render_layers, filter_mode, boundary_mode, f32)
    idx = np.where(st["empty"][..., None], -1, st["idx"])
    B, H, W, L = idx.shape[:4]
    best = None
    for b in range(B):
        for y in range(0, H, tile):
            for x in range(0, W, tile):
                for l in range(L):
                    k = np.unique(idx[b, y:y + tile, x:x + tile, l])
                    n = int((k >= 0).sum())
                    best = n if best is None else worst(best, n)
    return best


# ---- "every instantiation once": the smallest inputs at which each loop of the kernels still has two iterations and each guard
# both outcomes (two views, four 16 x 16 tiles per view of which three are partial, two layers), shared by the three texture ops
INST_SHAPE = (2, 17, 17, 2)               # B, H, W, L
INST_CS = (1, 2, 3, 4, 5, 8)              # the scatter's chunk 1, 2, 3; 4 exact; 4 with a tail chunk; two float4 groups


def instantiation_ids(seed=0):
    """render_layers (B,H,W,L) int32: about a quarter negative; at the one-pixel corner tile view 0 is live and view 1 empty."""
    rng = np.random.default_rng(seed)
    rl = np.where(rng.uniform(size=INST_SHAPE) < 0.25, -1, rng.integers(0, 9, INST_SHAPE)).astype(np.int32)
    rl[0, 16, 16], rl[1, 16, 16] = 3, -1
    return rl


def spoil(coords, rl, seed=0, n=6):
    """NaN, +inf and -inf into one component of ``n`` live slots' coordinates (not the corner pixel's) -> the spoilt slots."""
    rng = np.random.default_rng(seed + 1)
    live = np.argwhere((rl >= 0) & ~((np.arange(17)[:, None] == 16) & (np.arange(17)[None, :] == 16))[None, :, :, None])
    pick = live[rng.choice(len(live), n, replace=False)]
    for k, p in enumerate(pick):
        coords[tuple(p) + (k % coords.shape[-1],)] = (np.nan, np.inf, -np.inf)[k % 3]
    return pick


def instantiation_case(seed=0):
    """-> (uv (B,H,W,L,2) uniform in [-0.5, 1.5]^2 with a few NaN and infinite entries, render_layers)."""
    rl = instantiation_ids(seed)
    uv = np.random.default_rng(seed + 2).uniform(-0.5, 1.5, INST_SHAPE + (2,)).astype(f32)
    spoil(uv, rl, seed)
    return uv, rl


def tiles_have_live_and_empty(empty, tile=16):
    """Every tile of every layer holds live and empty slots: in each view where the tile has more than one pixel, and over the
    views where it is a single pixel (one slot per view and layer cannot be both)."""
    B, H, W, L = empty.shape
    for y, x, l in ((y, x, l) for y in range(0, H, tile) for x in range(0, W, tile) for l in range(L)):
        t = empty[:, y:y + tile, x:x + tile, l]
        groups = [t] if t[0].size == 1 else list(t)
        if not all(g.any() and not g.all() for g in groups):
            return False
    return True
