"""Restatement of the hash grid contract of Renderer.hash_grid (include/dm2_hip.h: dm2_hash_grid / dm2_hash_grid_backward)
in numpy.

xyz (B,H,W,L,3) = a position per slot in the field's unit cube; table (NL,T,F), T a power of two; render_layers (B,H,W,L) or None;
N the base resolution, q = 16 growth in 17..32.  Level resolutions R_0 = N, R_{l+1} = (R_l q) >> 4.  Per slot and level, in float32:

    X = x R_l - 0.5    X0 = floor(X)    fx = X - X0    i0 = int(X0)         (Y, fy, j0 and Z, fz, k0 alike)

A slot is empty when its id is negative or |X|, |Y| or |Z| at the finest level is not below 2^24 (NaN and infinite coordinates
included): zeros in all NL F channels, no gradient, nothing read through it.  Otherwise the taps of level l are
t_pqr = table[l][row(addr(k0 + r), addr(j0 + q), addr(i0 + p))], tap number p + 2 q + 4 r, addr = clip to [0, R_l - 1] (clamp) or
mod R_l (wrap), row = (k R_l + j) R_l + i where R_l^3 <= T and (i ^ j 2654435761 ^ k 805459861) mod 2^32 mod T otherwise, and

    b_qr = t_0qr + fx (t_1qr - t_0qr)    a_r = b_0r + fy (b_1r - b_0r)    out[l F + f] = a_0 + fz (a_1 - a_0)

nearest takes the voxel (addr(floor(Z + 0.5)), addr(floor(Y + 0.5)), addr(floor(X + 0.5))).
"""
import numpy as np

f32 = np.float32
FILTERS = ("nearest", "linear")
BOUNDARIES = ("clamp", "wrap")
RANGE = 16777216.0
PRIME_J, PRIME_K = 2654435761, 805459861


def resolutions(NL, N, q):
    """[R_0, ..., R_{NL-1}]."""
    assert 17 <= q <= 32 and NL >= 1 and N >= 1
    res = [int(N)]
    while len(res) < NL:
        res.append((res[-1] * int(q)) >> 4)
    return res


def is_dense(R, T):
    return R ** 3 <= T


def rows(i, j, k, R, T):
    """Table rows of the voxels (k, j, i) (integer arrays, addresses after addr) of a level of resolution R -> int64."""
    i, j, k = (np.asarray(a).astype(np.int64) for a in (i, j, k))
    if is_dense(R, T):
        return (k * R + j) * R + i
    u = np.uint32
    with np.errstate(over="ignore"):
        h = i.astype(u) ^ (j.astype(u) * u(PRIME_J)) ^ (k.astype(u) * u(PRIME_K))
    return (h & u(T - 1)).astype(np.int64)


def _addr(i, n, boundary_mode):
    return np.clip(i, 0, n - 1) if boundary_mode == "clamp" else np.mod(i, n)


def _out_of_range(p, R, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        X = ((p * dtype(R)).astype(dtype) - dtype(0.5)).astype(dtype)
        return ~(np.abs(X) < dtype(RANGE)).all(-1)


def empty(xyz, res, render_layers=None, any_level=False, dtype=f32):
    """(B,H,W,L) bool: the empty slots for the level resolutions ``res`` (the same for both filters and boundaries): the range
    rule at the finest level; ``any_level``: at any level."""
    p = np.asarray(xyz).astype(dtype)
    e = _out_of_range(p, res[-1], dtype)
    if any_level:
        for R in res[:-1]:
            e = e | _out_of_range(p, R, dtype)
    if render_layers is not None:
        e = e | (np.asarray(render_layers) < 0)
    return e


def stage(xyz, res, T, render_layers, filter_mode, boundary_mode, dtype=f32):
    """The contract's first stage in ``dtype`` (float32: the contract itself) -> dict(empty (B,H,W,L) bool, f (NL,B,H,W,L,3) =
    (fx, fy, fz) per level, rows (NL,B,H,W,L,8) int64 = the table row of tap p + 2 q + 4 r per level (nearest: the one row eight
    times); zeros in empty slots)."""
    if filter_mode not in FILTERS:
        raise ValueError(filter_mode)
    if boundary_mode not in BOUNDARIES:
        raise ValueError(boundary_mode)
    p = np.asarray(xyz).astype(dtype)
    e = empty(p, res, render_layers, dtype=dtype)
    fs, rs = [], []
    for R in res:
        with np.errstate(invalid="ignore", over="ignore"):
            X = ((p * dtype(R)).astype(dtype) - dtype(0.5)).astype(dtype)
        X = np.where(e[..., None], dtype(0), X).astype(dtype)
        if filter_mode == "nearest":
            c = [_addr(np.floor((X[..., a] + dtype(0.5)).astype(dtype)).astype(np.int64), R, boundary_mode) for a in range(3)]
            r = np.repeat(rows(c[0], c[1], c[2], R, T)[..., None], 8, -1)
            f = np.zeros(X.shape, dtype)
        else:
            X0 = np.floor(X)
            f = (X - X0).astype(dtype)
            c0 = X0.astype(np.int64)
            ad = [[_addr(c0[..., a] + d, R, boundary_mode) for d in (0, 1)] for a in range(3)]
            r = np.stack([rows(ad[0][pp], ad[1][qq], ad[2][rr], R, T) for rr in (0, 1) for qq in (0, 1) for pp in (0, 1)], -1)
        fs.append(np.where(e[..., None], dtype(0), f).astype(dtype))
        rs.append(np.where(e[..., None], 0, r))
    return dict(empty=e, f=np.stack(fs), rows=np.stack(rs))


def forward(xyz, table, render_layers, N, q, filter_mode="linear", boundary_mode="clamp", dtype=f32):
    """The whole contract in ``dtype``: separate multiplies and adds, in the written order -> (B,H,W,L,NL*F)."""
    table = np.asarray(table)
    NL, T, F = table.shape
    st = stage(xyz, resolutions(NL, N, q), T, render_layers, filter_mode, boundary_mode, dtype)
    tab = table.astype(dtype, copy=False)
    outs = []
    for l in range(NL):
        r = st["rows"][l]
        if filter_mode == "nearest":
            o = tab[l][r[..., 0]]
        else:
            t = [tab[l][r[..., k]] for k in range(8)]                        # (B,H,W,L,F) each; an empty slot's rows are masked below
            fx, fy, fz = (st["f"][l][..., a, None] for a in range(3))
            with np.errstate(invalid="ignore", over="ignore"):
                lerp = lambda u, v, w: (u + (w * (v - u).astype(dtype)).astype(dtype)).astype(dtype)
                a = [lerp(lerp(t[4 * rr], t[4 * rr + 1], fx), lerp(t[4 * rr + 2], t[4 * rr + 3], fx), fy) for rr in (0, 1)]
                o = lerp(a[0], a[1], fz)
        outs.append(o)
    out = np.concatenate(outs, -1)
    return np.where(st["empty"][..., None], dtype(0), out).astype(dtype)


def forward32(xyz, table, render_layers, N, q, filter_mode="linear", boundary_mode="clamp"):
    return forward(xyz, table, render_layers, N, q, filter_mode, boundary_mode, f32)


def forward64(xyz, table, render_layers, N, q, filter_mode="linear", boundary_mode="clamp"):
    return forward(xyz, table, render_layers, N, q, filter_mode, boundary_mode, np.float64)


def _weights64(f, filter_mode):
    """float64 -> (w (...,8) = d out / d t_k, dw (3, ...,8) = d w_k / d f_a) at the fractions f (...,3)."""
    shape = f.shape[:-1]
    if filter_mode == "nearest":
        w = np.zeros(shape + (8,))
        w[..., 0] = 1.0
        return w, np.zeros((3,) + shape + (8,))
    f = f.astype(np.float64)
    ax = [np.stack([1.0 - f[..., a], f[..., a]], -1) for a in range(3)]
    dax = [np.stack([-np.ones(shape), np.ones(shape)], -1) for a in range(3)]
    order = [(k & 1, (k >> 1) & 1, (k >> 2) & 1) for k in range(8)]
    w = np.stack([ax[0][..., p] * ax[1][..., q] * ax[2][..., r] for p, q, r in order], -1)
    dw = np.stack([np.stack([(dax[0] if a == 0 else ax[0])[..., p] * (dax[1] if a == 1 else ax[1])[..., q] *
                             (dax[2] if a == 2 else ax[2])[..., r] for p, q, r in order], -1) for a in range(3)])
    return w, dw


def grads64(xyz, table, render_layers, N, q, filter_mode, boundary_mode, g, stage_dtype=f32, absolute=False):
    """(dL/dtable (NL,T,F), dL/dxyz (B,H,W,L,3)) for upstream g (B,H,W,L,NL*F): fractions and rows from the float32 stage,
    everything after in float64 (the derivative of the float32 function at its own fractions).
    ``stage_dtype=np.float64``: of the float64 function (what central differences of forward64 see).
    ``absolute``: every term of both sums by its absolute value (sum_s |w_k g| per table element; sum_l R_l sum_f sum_k
    |g dw_k t_k| per coordinate): what an fp32 evaluation's rounding error scales with, whatever its order."""
    table = np.asarray(table)
    NL, T, F = table.shape
    res = resolutions(NL, N, q)
    st = stage(xyz, res, T, render_layers, filter_mode, boundary_mode, stage_dtype)
    live = ~st["empty"]
    g = np.where(live[..., None], np.asarray(g).astype(np.float64), 0.0).reshape(live.shape + (NL, F))
    dtable = np.zeros((NL, T, F), np.float64)
    dxyz = np.zeros(live.shape + (3,), np.float64)
    for l in range(NL):
        r = st["rows"][l]
        w, dw = _weights64(st["f"][l], filter_mode)
        w = np.where(live[..., None], w, 0.0)
        t = np.where(live[..., None, None], table[l][r].astype(np.float64), 0.0)      # (B,H,W,L,8,F); an empty slot's rows may hold NaN
        gl = g[..., l, :]
        if absolute:
            gl, w, dw, t = np.abs(gl), np.abs(w), np.abs(dw), np.abs(t)
        dxyz += np.stack([float(res[l]) * ((dw[a][..., None] * t).sum(-2) * gl).sum(-1) for a in range(3)], -1)
        flat = r.reshape(-1)
        for f in range(F):
            dtable[l, :, f] = np.bincount(flat, weights=(w * gl[..., f, None]).reshape(-1), minlength=T)
    return dtable, np.where(live[..., None], dxyz, 0.0)


def terms_abs(xyz, table, render_layers, N, q, filter_mode, boundary_mode, g):
    """(sum|terms| per element of dL/dtable, per element of dL/dxyz): util.summation_bound's second argument."""
    return grads64(xyz, table, render_layers, N, q, filter_mode, boundary_mode, g, absolute=True)


def distinct_rows_per_tile(xyz, R, T, render_layers=None, filter_mode="linear", boundary_mode="clamp", tile=16, worst=min):
    """The smallest (``worst=max``: the largest) number of distinct rows the non-empty slots of one layer address at a level of
    resolution R, over the tile x tile pixel tiles of every view and over the layers: against the scatter's table capacity it
    says which route a tile takes."""
    st = stage(xyz, [R], T, render_layers, filter_mode, boundary_mode, f32)
    idx = np.where(st["empty"][..., None], -1, st["rows"][0])
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
