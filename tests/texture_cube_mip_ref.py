"""Restatement of texture(filter_mode="linear-mipmap-linear", boundary_mode="cube", mip_level=...) (include/dm2_hip.h:
dm2_texture_cube_mip / dm2_texture_cube_mip_backward) in numpy, on tests/texture_cube_ref.py's stage / blend per
level and tests/texture_mip_ref.py's layout.

dirs (B,H,W,L,3); level (B,H,W,L) = the level of detail per slot; tex (6,N,N,C) or (B,6,N,N,C) = level 0; mip (6,T,C) or
(B,6,T,C) = per face the levels 1 .. nlev-1 in layout(N)'s packing, level k with faces of N_k = N >> k.  A slot is empty by
the cube op's rules or where its level is not finite.  lod <= 0: level 0 alone; lod >= nlev - 1: the last level alone;
otherwise j = floor(lod), f = lod - j, out = c_j + f (c_{j+1} - c_j), c_k = texture_cube_ref's linear sample of level k.
"""
import numpy as np

import texture_cube_ref as cref
import texture_mip_ref as mref

f32 = np.float32


def layout(N, max_mip_level=None):
    """-> (nlev, [(N_k, N_k, offset_k)], T) of one face: texture_mip_ref.layout(N, N)."""
    return mref.layout(N, N, max_mip_level)


def box_chain(tex, max_mip_level=None, dtype=f32):
    """The chain of 2 x 2 means within each face: tex (6,N,N,C) -> (6,T,C), (B,6,N,N,C) -> (B,6,T,C) (texture_mipmaps'
    restatement with the faces as leading dimensions)."""
    return mref.mipmaps(tex, max_mip_level, dtype)


def level_cube(tex, mip, k, max_mip_level=None):
    """Level k as a cube (6,N_k,N_k,C) or (B,6,N_k,N_k,C)."""
    return mref.level(tex, mip, k, max_mip_level)


def stage(dirs, level, N, render_layers=None, max_mip_level=None, dtype=f32):
    """The first stage -> dict(empty (B,H,W,L) bool, lod, j int (the first level), two bool (level j + 1 blends in), f (0 where
    not two), nlev), the level's arithmetic in ``dtype`` (float32: the contract)."""
    nlev, _, _ = layout(N, max_mip_level)
    lod = np.asarray(level).astype(dtype)
    empty = cref.empty(dirs, render_layers) | ~np.isfinite(lod)
    lod = np.where(empty, dtype(0), lod).astype(dtype)
    low, high = lod <= dtype(0), lod >= dtype(nlev - 1)
    two = ~empty & ~low & ~high
    jf = np.floor(lod)
    j = np.where(low, 0, np.where(high, nlev - 1, np.clip(jf, 0, nlev).astype(np.int64)))
    f = np.where(two, (lod - jf).astype(dtype), dtype(0)).astype(dtype)
    return dict(empty=empty, lod=lod, j=np.where(empty, 0, j), two=two, f=f, nlev=nlev)


def _ids(st):
    return np.where(st["empty"], -1, 0).astype(np.int32)


def _users(st, k):
    """(first, second): the slots whose level j, and whose level j + 1, is k."""
    return ~st["empty"] & (st["j"] == k), st["two"] & (st["j"] + 1 == k)


def level_stages(dirs, st, N, stage_dtype=f32):
    """{k: texture_cube_ref.stage at N_k of the slots that use level k} (the others empty)."""
    out = {}
    for k in range(st["nlev"]):
        first, second = _users(st, k)
        if first.any() or second.any():
            out[k] = cref.stage(dirs, N >> k, np.where(first | second, 0, -1).astype(np.int32), "linear", stage_dtype)
    return out


def samples(dirs, level, tex, mip, render_layers=None, max_mip_level=None, dtype=f32, stage_dtype=None, st=None):
    """-> (st, c_j, c_{j+1}) (B,H,W,L,C) in ``dtype`` (c_{j+1} zeros where one level is sampled); fractions and addresses of
    each level in ``stage_dtype`` (default ``dtype``)."""
    tex = np.asarray(tex)
    N, C = tex.shape[-2], tex.shape[-1]
    sd = stage_dtype or dtype
    if st is None:
        st = stage(dirs, level, N, render_layers, max_mip_level, sd)
    cj = np.zeros(st["j"].shape + (C,), dtype)
    cj1 = np.zeros_like(cj)
    for k, sk in level_stages(dirs, st, N, sd).items():
        first, second = _users(st, k)
        ck = cref.blend(sk, level_cube(tex, mip, k, max_mip_level), "linear", dtype)
        cj = np.where(first[..., None], ck, cj)
        cj1 = np.where(second[..., None], ck, cj1)
    return st, cj, cj1


def forward(dirs, level, tex, mip, render_layers=None, max_mip_level=None, dtype=f32, stage_dtype=None, st=None):
    """The whole contract in ``dtype``: separate multiplies and adds, in the written order."""
    st, cj, cj1 = samples(dirs, level, tex, mip, render_layers, max_mip_level, dtype, stage_dtype, st)
    with np.errstate(invalid="ignore", over="ignore"):
        f = st["f"].astype(dtype)[..., None]
        both = (cj + (f * (cj1 - cj).astype(dtype)).astype(dtype)).astype(dtype)
    out = np.where(st["two"][..., None], both, cj)
    return np.where(st["empty"][..., None], dtype(0), out).astype(dtype)


def forward32(dirs, level, tex, mip, render_layers=None, max_mip_level=None):
    return forward(dirs, level, tex, mip, render_layers, max_mip_level, f32)


def forward64(dirs, level, tex, mip, render_layers=None, max_mip_level=None):
    """The float64 function: what central differences see."""
    return forward(np.asarray(dirs, np.float64), np.asarray(level, np.float64), np.asarray(tex, np.float64), np.asarray(mip, np.float64),
                   render_layers, max_mip_level, np.float64)


def grads64(dirs, level, tex, mip, render_layers, max_mip_level, g, stage_dtype=f32):
    """(dL/dtex, dL/dmip, dL/ddirs (B,H,W,L,3), dL/dlevel (B,H,W,L), level_terms (B,H,W,L)) float64 for upstream g (B,H,W,L,C):
    lod, j, f, fractions, faces and addresses from the ``stage_dtype`` stage (float32: the derivative of the float32 function
    at its own values), everything after in float64.  Level k receives texture_cube_ref.grads64 of (1 - f) g, f g or g;
    dL/dlevel = sum_c g_c (c_{j+1,c} - c_{j,c}) where two levels blend; level_terms = sum_c |g_c| (|c_j| + |c_{j+1}|) there:
    what the rounding of that difference scales with."""
    tex, mip = np.asarray(tex), np.asarray(mip)
    N, C = tex.shape[-2], tex.shape[-1]
    st = stage(dirs, level, N, render_layers, max_mip_level, stage_dtype)
    _, levels, _ = layout(N, max_mip_level)
    g = np.asarray(g, np.float64)
    f = st["f"].astype(np.float64)
    dtex, dmip = np.zeros(tex.shape, np.float64), np.zeros(mip.shape, np.float64)
    ddir = np.zeros(st["j"].shape + (3,), np.float64)
    for k in range(st["nlev"]):
        first, second = _users(st, k)
        m = np.where(first, np.where(st["two"], 1.0 - f, 1.0), 0.0) + np.where(second, f, 0.0)
        if not (first.any() or second.any()):
            continue
        rl = np.where(first | second, 0, -1).astype(np.int32)
        dk, dd = cref.grads64(dirs, level_cube(tex, mip, k, max_mip_level), rl, "linear", g * m[..., None], stage_dtype)
        ddir += dd
        if k == 0:
            dtex += dk
        else:
            n, _, off = levels[k]
            dmip[..., off:off + n * n, :] += dk.reshape(mip.shape[:-2] + (n * n, C))
    _, cj, cj1 = samples(dirs, level, tex.astype(np.float64), mip.astype(np.float64), render_layers, max_mip_level, np.float64,
                         stage_dtype, st)
    two = st["two"]
    dlevel = np.where(two, (g * (cj1 - cj)).sum(-1), 0.0)
    terms = np.where(two, (np.abs(g) * (np.abs(cj) + np.abs(cj1))).sum(-1), 0.0)
    return dtex, dmip, ddir, dlevel, terms


def level_keys(idx, N, k, max_mip_level=None):
    """texture_cube_ref's flat texel indices (face N_k + j) N_k + i of level k in the kernel's key space of one view."""
    _, levels, T = layout(N, max_mip_level)
    n, _, off = levels[k]
    idx = np.asarray(idx, np.int64)
    return idx if k == 0 else 6 * N * N + (idx // (n * n)) * T + off + idx % (n * n)


def keys(dirs, level, N, render_layers=None, max_mip_level=None):
    """(B,H,W,L,8) int64: each slot's taps in the kernel's key space of one view (level 0: (face N + j) N + i, level k >= 1:
    6 N N + face T + offset_k + j N_k + i), level j's four, then level j + 1's; -1 in an empty slot, for a corner's missing tap
    and, where one level is sampled, in the second four."""
    st = stage(dirs, level, N, render_layers, max_mip_level)
    out = np.full(st["j"].shape + (8,), -1, np.int64)
    for k, sk in level_stages(dirs, st, N).items():
        first, second = _users(st, k)
        idx = np.where(np.arange(4) == sk["miss"][..., None], -1, level_keys(sk["idx"], N, k, max_mip_level))
        out[..., :4] = np.where(first[..., None], idx, out[..., :4])
        out[..., 4:] = np.where(second[..., None], idx, out[..., 4:])
    return out


def distinct_keys_per_tile(dirs, level, N, render_layers=None, max_mip_level=None, tile=16, worst=min):
    """The smallest (``worst=max``: the largest) number of distinct keys the slots of one layer address, over the tile x tile
    pixel tiles of every view and over the layers."""
    ks = keys(dirs, level, N, render_layers, max_mip_level)
    B, H, W, L = ks.shape[:4]
    best = None
    for b in range(B):
        for y in range(0, H, tile):
            for x in range(0, W, tile):
                for l in range(L):
                    k = np.unique(ks[b, y:y + tile, x:x + tile, l])
                    n = int((k >= 0).sum())
                    best = n if best is None else worst(best, n)
    return best


def _step(a, n):
    a = f32(a)
    for _ in range(abs(n)):
        a = np.nextafter(a, f32(np.inf) if n > 0 else f32(-np.inf))
    return a


def level_edges(nlev):
    """float32 levels on and next to every branch point: every integer 0 .. nlev and the floats next to each on either side,
    +-0, a denormal, 1e30 and its negative, then NaN and +-inf (empty slots)."""
    rows = []
    for k in range(nlev + 1):
        rows += [f32(k), _step(k, -1), _step(k, 1)]
    rows += [f32(0.0), f32(-0.0), f32(1e-45), f32(-1e-45), f32(1e30), f32(-1e30), f32(np.nan), f32(np.inf), f32(-np.inf)]
    return np.array(rows, f32)
