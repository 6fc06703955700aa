"""Restatement of the volume contract of Renderer.texture3d (include/dm2_hip.h: dm2_texture_volume /
dm2_texture_volume_backward) in numpy.

xyz (B,H,W,L,3) = a position per slot in the grid's unit cube, x along the grid's last spatial axis and z along its first; grid
(N,N,N,C) shared by the views or (B,N,N,N,C), indexed [k][j][i]; render_layers (B,H,W,L) or None.  Per slot, in float32:

    X = x N - 0.5    X0 = floor(X)    fx = X - X0    i0 = int(X0)         (Y, fy, j0 and Z, fz, k0 alike)

A slot is empty when its id is negative or |X|, |Y| or |Z| is not below 2^24 (NaN and infinite coordinates included): zeros
out, no gradient, nothing read through it.  Otherwise the taps are t_pqr = grid[addr(k0 + r)][addr(j0 + q)][addr(i0 + p)], tap
number p + 2 q + 4 r, addr = clip to [0, N - 1] (clamp) or mod N (wrap), and

    b_qr = t_0qr + fx (t_1qr - t_0qr)    a_r = b_0r + fy (b_1r - b_0r)    out = a_0 + fz (a_1 - a_0)

nearest takes the voxel (addr(floor(Z + 0.5)), addr(floor(Y + 0.5)), addr(floor(X + 0.5))).
"""
import numpy as np

f32 = np.float32
FILTERS = ("nearest", "linear")
BOUNDARIES = ("clamp", "wrap")
RANGE = 16777216.0


def _addr(i, N, boundary_mode):
    return np.clip(i, 0, N - 1) if boundary_mode == "clamp" else np.mod(i, N)


def stage(xyz, N, render_layers, filter_mode, boundary_mode, dtype=f32):
    """The contract's first stage in ``dtype`` (float32: the contract itself) -> dict(empty (B,H,W,L) bool, X (B,H,W,L,3) the
    voxel-space coordinates, f (B,H,W,L,3) = (fx, fy, fz), idx (B,H,W,L,8) int64 = flat voxel (k N + j) N + i of tap p + 2 q + 4 r
    (nearest: the one voxel eight times); zeros in empty slots)."""
    if filter_mode not in FILTERS:
        raise ValueError(filter_mode)
    if boundary_mode not in BOUNDARIES:
        raise ValueError(boundary_mode)
    p = np.asarray(xyz).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        X = ((p * dtype(N)).astype(dtype) - dtype(0.5)).astype(dtype)
        e = ~(np.abs(X) < dtype(RANGE)).all(-1)
    if render_layers is not None:
        e = e | (np.asarray(render_layers) < 0)
    X = np.where(e[..., None], dtype(0), X).astype(dtype)
    if filter_mode == "nearest":
        c = [_addr(np.floor((X[..., a] + dtype(0.5)).astype(dtype)).astype(np.int64), N, boundary_mode) for a in range(3)]
        idx = np.repeat(((c[2] * N + c[1]) * N + c[0])[..., None], 8, -1)
        f = np.zeros(X.shape, dtype)
    else:
        X0 = np.floor(X)
        f = (X - X0).astype(dtype)
        c0 = X0.astype(np.int64)
        ad = [[_addr(c0[..., a] + d, N, boundary_mode) for d in (0, 1)] for a in range(3)]
        idx = np.stack([(ad[2][r] * N + ad[1][q]) * N + ad[0][p] for r in (0, 1) for q in (0, 1) for p in (0, 1)], -1)
    return dict(empty=e, X=X, f=np.where(e[..., None], dtype(0), f).astype(dtype), idx=np.where(e[..., None], 0, idx))


def empty(xyz, N, render_layers=None):
    """(B,H,W,L) bool: the empty slots (the same for both filters and boundaries)."""
    return stage(xyz, N, render_layers, "nearest", "clamp")["empty"]


def _flat_idx(idx, grid):
    """Rows of grid.reshape(-1, C) for the (B,H,W,L,8) voxel indices (the view's own grid for a (B,N,N,N,C) one)."""
    if grid.ndim == 5:
        per = grid.shape[1] * grid.shape[2] * grid.shape[3]
        return idx + (np.arange(idx.shape[0], dtype=np.int64) * per).reshape(-1, 1, 1, 1, 1)
    return idx


def forward(xyz, grid, render_layers=None, filter_mode="linear", boundary_mode="clamp", dtype=f32):
    """The whole contract in ``dtype``: separate multiplies and adds, in the written order."""
    grid = np.asarray(grid)
    st = stage(xyz, grid.shape[-2], render_layers, filter_mode, boundary_mode, dtype)
    live_rows = np.where(st["empty"][..., None], 0, _flat_idx(st["idx"], grid))
    flat = grid.astype(dtype, copy=False).reshape(-1, grid.shape[-1])
    if filter_mode == "nearest":
        out = flat[live_rows[..., 0]]
    else:
        t = [flat[live_rows[..., k]] for k in range(8)]                     # (B,H,W,L,C) each; an empty slot's rows are masked below
        fx, fy, fz = (st["f"][..., a, None] for a in range(3))
        with np.errstate(invalid="ignore", over="ignore"):
            lerp = lambda u, v, w: (u + (w * (v - u).astype(dtype)).astype(dtype)).astype(dtype)
            a = [lerp(lerp(t[4 * r], t[4 * r + 1], fx), lerp(t[4 * r + 2], t[4 * r + 3], fx), fy) for r in (0, 1)]
            out = lerp(a[0], a[1], fz)
    return np.where(st["empty"][..., None], dtype(0), out).astype(dtype)


def forward32(xyz, grid, render_layers=None, filter_mode="linear", boundary_mode="clamp"):
    return forward(xyz, grid, render_layers, filter_mode, boundary_mode, f32)


def forward64(xyz, grid, render_layers=None, filter_mode="linear", boundary_mode="clamp"):
    return forward(xyz, grid, render_layers, filter_mode, boundary_mode, np.float64)


def _weights64(st, filter_mode):
    """float64 -> (w (B,H,W,L,8) = d out / d t_k, dw (3, B,H,W,L,8) = d w_k / d f_a) at ``stage``'s fractions."""
    shape = st["empty"].shape
    if filter_mode == "nearest":
        w = np.zeros(shape + (8,))
        w[..., 0] = 1.0
        return w, np.zeros((3,) + shape + (8,))
    f = st["f"].astype(np.float64)
    ax = [np.stack([1.0 - f[..., a], f[..., a]], -1) for a in range(3)]     # (B,H,W,L,2) per axis
    dax = [np.stack([-np.ones(shape), np.ones(shape)], -1) for a in range(3)]
    order = [(k & 1, (k >> 1) & 1, (k >> 2) & 1) for k in range(8)]
    w = np.stack([ax[0][..., p] * ax[1][..., q] * ax[2][..., r] for p, q, r in order], -1)
    dw = np.stack([np.stack([(dax[0] if a == 0 else ax[0])[..., p] * (dax[1] if a == 1 else ax[1])[..., q] *
                             (dax[2] if a == 2 else ax[2])[..., r] for p, q, r in order], -1) for a in range(3)])
    return w, dw


def grads64(xyz, grid, render_layers, filter_mode, boundary_mode, g, stage_dtype=f32, absolute=False):
    """(dL/dgrid of grid's shape, dL/dxyz (B,H,W,L,3)) for upstream g (B,H,W,L,C): fractions and addresses from the float32
    stage, everything after in float64 (the derivative of the float32 function at its own fractions).
    ``stage_dtype=np.float64``: of the float64 function (what central differences of forward64 see).
    ``absolute``: every term of both sums by its absolute value (sum_s |w_k g| per voxel element; N sum_c sum_k |g dw_k t_k| per
    coordinate): what an fp32 evaluation's rounding error scales with, whatever its order."""
    grid = np.asarray(grid)
    N, C = grid.shape[-2], grid.shape[-1]
    st = stage(xyz, N, render_layers, filter_mode, boundary_mode, stage_dtype)
    live = ~st["empty"]
    g = np.where(live[..., None], np.asarray(g).astype(np.float64), 0.0)
    rows = _flat_idx(st["idx"], grid)
    w, dw = _weights64(st, filter_mode)
    w = np.where(live[..., None], w, 0.0)
    t = grid.reshape(-1, C)[rows].astype(np.float64)                        # (B,H,W,L,8,C)
    t = np.where(live[..., None, None], t, 0.0)                             # (an empty slot's rows may hold NaN)
    if absolute:
        g, w, dw, t = np.abs(g), np.abs(w), np.abs(dw), np.abs(t)
    dxyz = np.stack([float(N) * ((dw[a][..., None] * t).sum(-2) * g).sum(-1) for a in range(3)], -1)
    dxyz = np.where(live[..., None], dxyz, 0.0)
    n = grid.size // C
    dgrid = np.zeros((n, C), np.float64)
    flat_rows = rows.reshape(-1)
    for c in range(C):
        dgrid[:, c] = np.bincount(flat_rows, weights=(w * g[..., c, None]).reshape(-1), minlength=n)
    return dgrid.reshape(grid.shape), dxyz


def terms_abs(xyz, grid, render_layers, filter_mode, boundary_mode, g):
    """(sum|terms| per element of dL/dgrid, per element of dL/dxyz): util.summation_bound's second argument."""
    return grads64(xyz, grid, render_layers, filter_mode, boundary_mode, g, absolute=True)


def distinct_voxels_per_tile(xyz, N, render_layers=None, filter_mode="linear", boundary_mode="clamp", tile=16, worst=min):
    """The smallest (``worst=max``: the largest) number of distinct voxels the non-empty slots of one layer address, over the
    tile x tile pixel tiles of every view and over the layers: against the scatter's table capacity it says which route a tile
    takes."""
    st = stage(xyz, N, render_layers, filter_mode, boundary_mode, f32)
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
