"""Restatement of the cube-map contract of Renderer.texture(boundary_mode="cube") (include/dm2_hip.h: dm2_texture_cube /
dm2_texture_cube_backward) in numpy.

dirs (B,H,W,L,3) = a direction per slot, any non-zero length; tex (6,N,N,C) shared by the views or (B,6,N,N,C); render_layers
(B,H,W,L) or None.  A slot is empty when its id is negative, a component is not finite, or all three are zero: zeros out, no
gradient, nothing read through it.  Otherwise, with ax, ay, az = |x|, |y|, |z|:

    axis = x if ax >= ay and ax >= az, else y if ay >= az, else z;  face = 2 axis + (sign bit of the major component)
    (faces +x, -x, +y, -y, +z, -z);  ma = |major|;  (sc, tc) by the OpenGL table FACE_ST below
    s = 0.5 (sc / ma + 1)    t = 0.5 (tc / ma + 1)    x = s N - 0.5    y = t N - 0.5
    x0 = floor(x)   fx = x - x0   y0 = floor(y)   fy = y - y0     (x, y lie in [-0.5, N - 0.5])

nearest takes the face's texel (clamp(floor(x + 0.5)), clamp(floor(y + 0.5))).  linear takes the taps (i0 + p, j0 + q), tap
k = p + 2 q: a tap inside the face is that texel; a tap outside on one axis is the texel of the face across that border, in that
face's row or column along the shared edge at the same position along the edge; a tap outside on both axes (a cube corner) does
not exist.  With all four taps: a = t00 + fx (t10 - t00), b = t01 + fx (t11 - t01), out = a + fy (b - a).  With tap m missing:
gx = 1 - fx, gy = 1 - fy, w = (gx gy, fx gy, gx fy, fx fy) with w_m = 0 and t_m = 0,
    W = ((w0 + w1) + w2) + w3,  out = (((w0 t0 + w1 t1) + w2 t2) + w3 t3) / W.

The seam table (which face lies across which border, which of its borders that is, whether the position along the edge runs
the other way) is DERIVED here from the cube's geometry (seam_table); the kernel carries it as a literal, and
tests/test_texture_cube_cpu.py compares the two.
"""
import numpy as np

import texture_ref as tref

f32 = np.float32
FILTERS = ("nearest", "linear")

# face -> ((axis of sc, sign), (axis of tc, sign)): the OpenGL table
FACE_ST = (((2, -1), (1, -1)),      # +x: sc = -z, tc = -y
           ((2, +1), (1, -1)),      # -x: sc = +z, tc = -y
           ((0, +1), (2, +1)),      # +y: sc = +x, tc = +z
           ((0, +1), (2, -1)),      # -y: sc = +x, tc = -z
           ((0, +1), (1, -1)),      # +z: sc = +x, tc = -y
           ((0, -1), (1, -1)))      # -z: sc = -x, tc = -y
# borders of a face: 0: i < 0 (s = 0), 1: i >= N (s = 1), 2: j < 0 (t = 0), 3: j >= N (t = 1)


def _point(face, sc, tc):
    """The point of the cube [-1, 1]^3 at face coordinates (sc, tc) of ``face``."""
    p = [0.0, 0.0, 0.0]
    p[face // 2] = -1.0 if face % 2 else 1.0
    (a, sa), (b, sb) = FACE_ST[face]
    p[a], p[b] = sa * sc, sb * tc                     # sc = sa * p[a]  <=>  p[a] = sa * sc
    return p


def _project(face, p):
    (a, sa), (b, sb) = FACE_ST[face]
    return sa * p[a], sb * p[b]


def seam_table():
    """((neighbour face, its border, reversed) per border) per face, from the geometry: two points of the border, at -1/2 and
    +1/2 along it, lie on exactly one other face; there one face coordinate is -1 or +1 (which border), and the other is the
    position along the edge, equal or negated."""
    table = []
    for f in range(6):
        row = []
        for e in range(4):
            fixed = -1.0 if e % 2 == 0 else 1.0
            pts = [_point(f, fixed, u) if e < 2 else _point(f, u, fixed) for u in (-0.5, 0.5)]
            others = [g for g in range(6) if g != f and all(p[g // 2] == (-1.0 if g % 2 else 1.0) for p in pts)]
            assert len(others) == 1
            g = others[0]
            (s0, t0), (s1, t1) = (_project(g, p) for p in pts)
            if s0 == s1:                              # the neighbour's left or right border: t runs along the edge
                assert abs(s0) == 1.0
                ne, along = (0 if s0 < 0 else 1), (t0, t1)
            else:
                assert t0 == t1 and abs(t0) == 1.0
                ne, along = (2 if t0 < 0 else 3), (s0, s1)
            assert along in ((-0.5, 0.5), (0.5, -0.5))
            row.append((g, ne, int(along == (0.5, -0.5))))
        table.append(tuple(row))
    return tuple(table)


SEAMS = seam_table()


def near_seams(rng, n, N, reach=0.6):
    """(2 n, 3) float64 directions for the tests: n within ``reach`` texels of one border of their face (edges; the other
    coordinate anywhere) and n within it of two (corners), from every face, border and corner, from inside the face, with
    lengths in [1/e, e]."""
    out = []
    for both in (False, True):
        f = rng.integers(0, 6, n)
        sgn = rng.choice([-1.0, 1.0], (n, 2))
        st = sgn * (1.0 - rng.uniform(0, reach, (n, 2)) * 2.0 / N)         # in sc units a texel is 2 / N wide
        if not both:
            st[np.arange(n), rng.integers(0, 2, n)] = rng.uniform(-1, 1, n)
        p = np.array([_point(int(ff), a, b) for ff, (a, b) in zip(f, st)])
        out.append(p * np.exp(rng.uniform(-1, 1, (n, 1))))
    return np.concatenate(out)


def exact_directions():
    """(6 + 12 * 5 + 8, 3) float64: the six axes, five points on each of the twelve edges (the midpoint among them), the eight
    corners; every component is 0, +-1 or a multiple of 1/4."""
    axes = [_point(f, 0.0, 0.0) for f in range(6)]
    edges = {tuple(_point(f, -1.0 if e % 2 == 0 else 1.0, u) if e < 2 else _point(f, u, -1.0 if e % 2 == 0 else 1.0))
             for f in range(6) for e in range(4) for u in (-0.75, -0.25, 0.0, 0.25, 0.75)}       # (a set: each edge comes up from both faces)
    corners = [(a, b, c) for a in (-1.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)]
    out = np.array(axes + sorted(edges) + corners)
    assert out.shape == (6 + 60 + 8, 3)
    return out


def _texel(N, face, i, j):
    """Flat texel index face N N + j N + i of tap (i, j) of ``face`` (int64 arrays) after the seam rule -> (index, on another
    face (bool), missing (bool)); the index of a missing tap is 0."""
    ox, oy = (i < 0) | (i >= N), (j < 0) | (j >= N)
    e = np.where(ox, np.where(i < 0, 0, 1), np.where(j < 0, 2, 3))
    k = np.where(ox, j, i)
    tab = np.asarray(SEAMS, np.int64)                                     # (6, 4, 3)
    nf, ne, rev = (tab[face, e, c] for c in range(3))
    kk = np.where(rev == 1, N - 1 - k, k)
    si = np.where(ne == 0, 0, np.where(ne == 1, N - 1, kk))
    sj = np.where(ne == 2, 0, np.where(ne == 3, N - 1, kk))
    seam, miss = ox ^ oy, ox & oy
    f2, i2, j2 = np.where(seam, nf, face), np.where(seam, si, i), np.where(seam, sj, j)
    return np.where(miss, 0, (f2 * N + j2) * N + i2), seam, miss


def stage(dirs, N, render_layers, filter_mode, dtype=f32, face=None):
    """The contract's first stage in ``dtype`` (float32: the contract itself) -> dict(empty (B,H,W,L) bool, face, sc, tc, ma, x,
    y, fx, fy, idx (B,H,W,L,4) int64 = flat texel of taps t00, t10, t01, t11 (nearest: the one texel four times), seam
    (B,H,W,L,4) bool: the tap lies on an adjacent face, miss (B,H,W,L) = the missing tap or -1, i0, j0 = tap 0's column and row
    on the face, -1 .. N - 1 (nearest: the texel's); zeros in empty slots).
    ``face`` (B,H,W,L) int: evaluate every slot as that face instead of the one the major axis picks (for the test that walks
    an edge from both sides; ma is then that face's axis component, which must not be zero)."""
    if filter_mode not in FILTERS:
        raise ValueError(filter_mode)
    d = np.asarray(dirs)
    comp = [d[..., k].astype(dtype) for k in range(3)]
    e = ~(np.isfinite(comp[0]) & np.isfinite(comp[1]) & np.isfinite(comp[2])) | ((comp[0] == 0) & (comp[1] == 0) & (comp[2] == 0))
    if render_layers is not None:
        e = e | (np.asarray(render_layers) < 0)
    comp = [np.where(e, dtype(1), c).astype(dtype) for c in comp]          # (placeholders; masked at the end)
    ax, ay, az = (np.abs(c) for c in comp)
    axis = np.where((ax >= ay) & (ax >= az), 0, np.where(ay >= az, 1, 2))
    major = np.where(axis == 0, comp[0], np.where(axis == 1, comp[1], comp[2]))
    fc = 2 * axis + np.signbit(major).astype(np.int64)
    if face is not None:
        fc = np.where(e, fc, np.asarray(face, np.int64))
    allc = np.stack(comp, -1)
    tab = np.asarray(FACE_ST, np.int64)                                   # (6, 2, 2)
    pick = lambda a: np.take_along_axis(allc, a[..., None], -1)[..., 0]
    ma = np.abs(pick(fc // 2)).astype(dtype)
    sc = (tab[fc, 0, 1].astype(dtype) * pick(tab[fc, 0, 0])).astype(dtype)
    tc = (tab[fc, 1, 1].astype(dtype) * pick(tab[fc, 1, 0])).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = (dtype(0.5) * ((sc / ma).astype(dtype) + dtype(1))).astype(dtype)
        t = (dtype(0.5) * ((tc / ma).astype(dtype) + dtype(1))).astype(dtype)
        x = ((s * dtype(N)).astype(dtype) - dtype(0.5)).astype(dtype)
        y = ((t * dtype(N)).astype(dtype) - dtype(0.5)).astype(dtype)
    if filter_mode == "nearest":
        i = np.clip(np.floor(x + dtype(0.5)).astype(np.int64), 0, N - 1)
        j = np.clip(np.floor(y + dtype(0.5)).astype(np.int64), 0, N - 1)
        idx = np.repeat(((fc * N + j) * N + i)[..., None], 4, -1)
        seam = np.zeros(idx.shape, bool)
        miss = np.full(x.shape, -1, np.int64)
        fx = fy = np.zeros(x.shape, dtype)
        i0, j0 = i, j
    else:
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0).astype(dtype), (y - y0).astype(dtype)
        i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
        taps = [_texel(N, fc, i0 + p, j0 + q) for q in (0, 1) for p in (0, 1)]
        idx = np.stack([a[0] for a in taps], -1)
        seam = np.stack([a[1] for a in taps], -1)
        m = np.stack([a[2] for a in taps], -1)
        assert (m.sum(-1) <= 1).all()
        miss = np.where(m.any(-1), m.argmax(-1), -1)
    z = lambda a: np.where(e, dtype(0), a).astype(dtype)
    return dict(empty=e, face=np.where(e, 0, fc), sc=z(sc), tc=z(tc), ma=z(ma), x=z(x), y=z(y), fx=z(fx), fy=z(fy),
                idx=np.where(e[..., None], 0, idx), seam=seam & ~e[..., None], miss=np.where(e, -1, miss),
                i0=np.where(e, 0, i0), j0=np.where(e, 0, j0))


def empty(dirs, render_layers=None):
    """(B,H,W,L) bool: the empty slots (the same for both filters and every N)."""
    return stage(dirs, 1, render_layers, "nearest")["empty"]


def _flat_idx(idx, tex):
    """Rows of tex.reshape(-1, C) for the (B,H,W,L,4) texel indices (the view's own cube for a (B,6,N,N,C) one)."""
    if tex.ndim == 5:
        per = 6 * tex.shape[2] * tex.shape[3]
        return idx + (np.arange(idx.shape[0], dtype=np.int64) * per).reshape(-1, 1, 1, 1, 1)
    return idx


def _weights(st, dtype):
    """-> (w (B,H,W,L,4) with the missing tap's weight 0, W (B,H,W,L)) in ``dtype``, the products and sums in the written order."""
    fx, fy = st["fx"].astype(dtype), st["fy"].astype(dtype)
    gx, gy = (dtype(1) - fx).astype(dtype), (dtype(1) - fy).astype(dtype)
    w = np.stack([(gx * gy).astype(dtype), (fx * gy).astype(dtype), (gx * fy).astype(dtype), (fx * fy).astype(dtype)], -1)
    w = np.where(np.arange(4) == st["miss"][..., None], dtype(0), w).astype(dtype)
    W = (((w[..., 0] + w[..., 1]).astype(dtype) + w[..., 2]).astype(dtype) + w[..., 3]).astype(dtype)
    return w, W


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
            corner = st["miss"] >= 0
            if corner.any():
                w, W = _weights(st, dtype)
                tm = np.where((np.arange(4) == st["miss"][..., None])[..., None], dtype(0), t).astype(dtype)
                p = [(w[..., k, None] * tm[..., k, :]).astype(dtype) for k in range(4)]
                acc = (((p[0] + p[1]).astype(dtype) + p[2]).astype(dtype) + p[3]).astype(dtype)
                out = np.where(corner[..., None], (acc / np.where(corner, W, dtype(1))[..., None]).astype(dtype), out)
    return np.where(st["empty"][..., None], dtype(0), out).astype(dtype)


def forward(dirs, tex, render_layers=None, filter_mode="linear", dtype=f32, face=None):
    """The whole contract in ``dtype``: separate multiplies and adds, in the written order."""
    tex = np.asarray(tex)
    return blend(stage(dirs, tex.shape[-2], render_layers, filter_mode, dtype, face), tex, filter_mode, dtype)


def forward32(dirs, tex, render_layers=None, filter_mode="linear", face=None):
    return forward(dirs, tex, render_layers, filter_mode, f32, face)


def forward64(dirs, tex, render_layers=None, filter_mode="linear", face=None):
    return forward(dirs, tex, render_layers, filter_mode, np.float64, face)


def tap_weights(st):
    """float64 (B,H,W,L,4): d out / d t_k of ``stage``'s output (nearest: 1 on tap 0; a missing tap: 0; corners renormalised)."""
    fx, fy = st["fx"].astype(np.float64), st["fy"].astype(np.float64)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1)
    w = np.where(np.arange(4) == st["miss"][..., None], 0.0, w)
    return w / w.sum(-1, keepdims=True)


def grads64(dirs, tex, render_layers, filter_mode, g, stage_dtype=f32):
    """(dL/dtex of tex's shape, dL/ddirs (B,H,W,L,3)) for upstream g (B,H,W,L,C): faces, fractions, addresses and sc, tc, ma
    from the float32 stage, everything after in float64 (the derivative of the float32 function at its own fractions).
    ``stage_dtype=np.float64``: of the float64 function (what central differences of forward64 see)."""
    tex = np.asarray(tex)
    N, C = tex.shape[-2], tex.shape[-1]
    st = stage(dirs, N, render_layers, filter_mode, stage_dtype)
    live = ~st["empty"]
    g = np.where(live[..., None], np.asarray(g).astype(np.float64), 0.0)
    rows = _flat_idx(st["idx"], tex)
    if filter_mode == "nearest":
        w = np.zeros(live.shape + (4,))
        w[..., 0] = 1.0
        ddir = np.zeros(live.shape + (3,))
    else:
        fx, fy = st["fx"].astype(np.float64), st["fy"].astype(np.float64)
        has = np.arange(4) != st["miss"][..., None]                        # (B,H,W,L,4)
        raw = np.where(has, np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1), 0.0)
        dwx = np.where(has, np.stack([-(1 - fy), 1 - fy, -fy, fy], -1), 0.0)
        dwy = np.where(has, np.stack([-(1 - fx), -fx, 1 - fx, fx], -1), 0.0)
        W = raw.sum(-1, keepdims=True)
        w = raw / W
        t = np.where(has[..., None], tex.reshape(-1, C)[rows].astype(np.float64), 0.0)            # (B,H,W,L,4,C)
        out = (w[..., None] * t).sum(-2)                                   # (B,H,W,L,C)
        rel = np.where(has[..., None], t - out[..., None, :], 0.0)
        dfx = ((dwx[..., None] * rel).sum(-2) * g).sum(-1) / W[..., 0]     # d out / d fx . g  (the quotient rule, with dW folded in)
        dfy = ((dwy[..., None] * rel).sum(-2) * g).sum(-1) / W[..., 0]
        A, Bq = 0.5 * N * dfx, 0.5 * N * dfy                               # dL/d(sc / ma), dL/d(tc / ma)
        sc, tc, ma = (st[k].astype(np.float64) for k in ("sc", "tc", "ma"))
        ma = np.where(live, ma, 1.0)
        dsc, dtc, dma = A / ma, Bq / ma, -(A * sc + Bq * tc) / (ma * ma)
        ddir = np.zeros(live.shape + (3,))
        tab = np.asarray(FACE_ST, np.int64)
        fc = st["face"]
        d = np.asarray(dirs).astype(np.float64)
        for k in range(3):
            ddir[..., k] += np.where(tab[fc, 0, 0] == k, tab[fc, 0, 1] * dsc, 0.0)
            ddir[..., k] += np.where(tab[fc, 1, 0] == k, tab[fc, 1, 1] * dtc, 0.0)
            ddir[..., k] += np.where(fc // 2 == k, np.where(np.signbit(np.where(live, d[..., k], 1.0)), -dma, dma), 0.0)
        ddir = np.where(live[..., None], ddir, 0.0)
    w = np.where(live[..., None], w, 0.0)
    n = tex.size // C
    dtex = np.zeros((n, C), np.float64)
    flat_rows = rows.reshape(-1)
    for c in range(C):
        dtex[:, c] = np.bincount(flat_rows, weights=(w * g[..., c, None]).reshape(-1), minlength=n)
    return dtex.reshape(tex.shape), ddir


def tex_terms_abs(dirs, tex, render_layers, filter_mode, g):
    """sum over the slots of |w_k g| per element of tex: what an fp32 sum's rounding error scales with, whatever its order."""
    tex = np.asarray(tex)
    return grads64(dirs, np.zeros_like(tex), render_layers, filter_mode, np.abs(np.asarray(g, np.float64)))[0]


def distinct_texels_per_tile(dirs, N, render_layers=None, filter_mode="linear", tile=16, worst=min):
    """The smallest (``worst=max``: the largest) number of distinct texels the non-empty slots of one layer address, over the
    tile x tile pixel tiles of every view and over the layers."""
    st = stage(dirs, N, render_layers, filter_mode, f32)
    idx = np.where(st["empty"][..., None] | (np.arange(4) == st["miss"][..., None]), -1, st["idx"])
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


INST_NS = (2, 5)


def instantiation_case(N, seed=0):
    """The "every instantiation once" inputs (texture_ref.INST_SHAPE, texture_ref.instantiation_ids) for an N x N cube ->
    (dirs (B,H,W,L,3) float32, render_layers): random directions, half of them replaced by near_seams' (aimed at the edges and
    corners of every face), a few NaN / infinite components."""
    rl = tref.instantiation_ids(seed)
    rng = np.random.default_rng(seed + 4 + N)
    d = rng.standard_normal((rl.size, 3))
    aimed = near_seams(rng, rl.size // 4, N)
    d[rng.choice(rl.size, len(aimed), replace=False)] = aimed
    d = d.reshape(tref.INST_SHAPE + (3,)).astype(f32)
    tref.spoil(d, rl, seed)
    return d, rl
