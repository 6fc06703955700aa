"""Restatement of Renderer.cube_prefilter (include/dm2_hip.h: dm2_cube_prefilter / dm2_cube_prefilter_backward) in numpy,
on tests/texture_cube_ref.py's face table and tests/texture_mip_ref.py's layout.

A level with faces of n x n has texels (face, j, i), row face n n + j n + i.  d, Om, K and the membership are computed in
float32 exactly as the contract writes them (separate multiplies and adds, in the written order); every sum is in float64.

    primitive:  y[o] = sum_s K(o,s) Om_s x[s]       transpose:  xbar[s] = Om_s sum_o K(o,s) ybar[o]
    cube_prefilter(tex) = primitive(box chain of tex) / primitive(ones)
"""
import functools

import numpy as np

import texture_cube_ref as cref
import texture_mip_ref as mref

f32 = np.float32
EPS = 2.0 ** -24


def layout(N, max_mip_level=None):
    """-> (nlev, [(n_k, n_k, offset_k)], T) of one face."""
    return mref.layout(N, N, max_mip_level)


def texels(n):
    """-> (d (6 n n, 3), Om (6 n n,)) float32: each texel's direction and its solid angle up to 4 / n^2."""
    c = ((f32(2) * (np.arange(n, dtype=f32) + f32(0.5))).astype(f32) / f32(n)).astype(f32) - f32(1)
    tc, sc = np.meshgrid(c, c, indexing="ij")                            # [j, i]
    q = ((f32(1) + (sc * sc).astype(f32)).astype(f32) + (tc * tc).astype(f32)).astype(f32)
    rq = np.sqrt(q).astype(f32)
    om = (f32(1) / (q * rq).astype(f32)).astype(f32)
    d = np.zeros((6, n, n, 3), f32)
    for face in range(6):
        p = [np.zeros((n, n), f32)] * 3
        p[face // 2] = np.full((n, n), -1.0 if face % 2 else 1.0, f32)
        (a, sa), (b, sb) = cref.FACE_ST[face]
        p[a], p[b] = (f32(sa) * sc).astype(f32), (f32(sb) * tc).astype(f32)      # cref._point, on arrays
        for k in range(3):
            d[face, :, :, k] = (p[k] / rq).astype(f32)
    return d.reshape(-1, 3), np.broadcast_to(om, (6, n, n)).reshape(-1).copy()


def roughness(k, nlev):
    """-> (r, a2) float32 of level k >= 1 of nlev levels."""
    r = f32(k) / f32(nlev - 1)
    a = f32(r * r)
    return r, f32(a * a)


def lobe(n, a2, rows=None):
    """-> (K (M,M) float32 with zeros off the members, member (M,M) bool), M = 6 n n, rows o, columns s; ``rows``: those rows
    o alone, (len(rows), M)."""
    a2 = f32(a2)
    d, _ = texels(n)
    do = d if rows is None else d[np.asarray(rows)]
    m = None
    for k in range(3):
        diff = (do[:, None, k] - d[None, :, k]).astype(f32)
        sq = (diff * diff).astype(f32)
        m = sq if m is None else (m + sq).astype(f32)
    c = (f32(1) - (f32(0.5) * m).astype(f32)).astype(f32)
    e = (a2 + ((f32(1) - a2).astype(f32) * (f32(0.25) * m).astype(f32)).astype(f32)).astype(f32)
    member = (c > 0) & (e <= f32(64) * a2)
    t = (a2 / e).astype(f32)
    K = ((t * t).astype(f32) * c).astype(f32)
    return np.where(member, K, f32(0)).astype(f32), member


@functools.lru_cache(maxsize=None)
def operator(n, k, nlev):
    """The forward's matrix of level k with faces of n: (A (M,M) float64 = K(o,s) Om_s, the products in float64 from the
    float32 factors; members per row (M,) int).  Cached: the tests share it and leave it unchanged."""
    K, member = lobe(n, roughness(k, nlev)[1])
    _, om = texels(n)
    A = K.astype(np.float64) * om.astype(np.float64)[None, :]
    A.setflags(write=False)
    return A, member.sum(1)


def _levels(chain, N, max_mip_level):
    """[(k, n, the level's texels as (..., 6 n n, C))] of a chain (..., 6, T, C)."""
    nlev, levels, T = layout(N, max_mip_level)
    chain = np.asarray(chain)
    assert chain.shape[-3:-1] == (6, T), (chain.shape, T)
    out = []
    for k in range(1, nlev):
        n, _, off = levels[k]
        out.append((k, n, chain[..., off:off + n * n, :].reshape(chain.shape[:-3] + (6 * n * n, chain.shape[-1]))))
    return nlev, out


def _pack(parts, shape, N, max_mip_level):
    nlev, levels, T = layout(N, max_mip_level)
    out = np.zeros(shape, np.float64)
    for (k, n, _), v in parts:
        off = levels[k][2]
        out[..., off:off + n * n, :] = v.reshape(shape[:-3] + (6, n * n, shape[-1]))
    return out


def primitive64(chain, N, max_mip_level=None, transpose=False):
    """The un-normalised filter (``transpose``: its transpose) of a chain (6,T,C) or (B,6,T,C) in float64 -> (y, terms = the
    same sums over absolute values, members (..., 6, T) = the terms of each sum): an element's fp32 sum in any order is held
    to (members + 4) 2^-24 terms."""
    chain = np.asarray(chain)
    nlev, lv = _levels(chain.astype(np.float64), N, max_mip_level)
    ys, ts, ms = [], [], []
    for k, n, x in lv:
        A, _ = operator(n, k, nlev)
        M = A.T if transpose else A
        ys.append(((k, n, None), M @ x))
        ts.append(((k, n, None), M @ np.abs(x)))
        cnt = (M != 0).sum(1).astype(np.float64)
        ms.append(((k, n, None), np.broadcast_to(cnt[:, None], x.shape)))
    shape = chain.shape
    return (_pack(ys, shape, N, max_mip_level), _pack(ts, shape, N, max_mip_level), _pack(ms, shape, N, max_mip_level)[..., 0])


def bound(terms, members):
    """The derived bound of an fp32 evaluation against primitive64: the products' roundings plus any order of the sum."""
    return (members[..., None] + 4.0) * EPS * terms


def norm64(N, max_mip_level=None):
    """W (6,T) float64 = primitive(ones), with its bound."""
    T = layout(N, max_mip_level)[2]
    y, terms, members = primitive64(np.ones((6, T, 1)), N, max_mip_level)
    return y[..., 0], bound(terms, members)[..., 0]


def prefilter64(tex, max_mip_level=None):
    """cube_prefilter in float64 from the float32 box chain (bit-exact in the package) -> (mip, tolerance): twice the
    primitive's bound over W (the numerator's and W's own) plus 4 * 2^-24 |mip| (the division and the quotient's rounding)."""
    tex = np.asarray(tex, f32)
    N = tex.shape[-2]
    chain = mref.mipmaps(tex, max_mip_level)
    y, terms, members = primitive64(chain, N, max_mip_level)
    W, _ = norm64(N, max_mip_level)
    out = y / W[..., None]
    return out, 2.0 * bound(terms, members) / W[..., None] + 4.0 * EPS * np.abs(out)


def prefilter_backward64(tex_shape, max_mip_level, g):
    """dL/dtex of cube_prefilter for upstream g of the chain's shape -> (grad, slack): g / W through the transpose and the box
    chain's backward in float64; slack = the transpose's bound pushed through the box chain's backward."""
    N = tex_shape[-2]
    W, _ = norm64(N, max_mip_level)
    gw = np.asarray(g, np.float64) / W[..., None]
    xbar, terms, members = primitive64(gw, N, max_mip_level, transpose=True)
    return (mref.mipmaps_backward64(tex_shape, max_mip_level, xbar),
            mref.mipmaps_backward64(tex_shape, max_mip_level, bound(terms, members)))
