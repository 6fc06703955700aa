"""Restatement of Renderer.texture_mipmaps and of texture(filter_mode="linear-mipmap-linear") (include/dm2_hip.h:
dm2_texture_mipmaps, dm2_texture_mip and their backwards) in numpy, on top of tests/texture_ref.py.

The chain: level 0 is the texture; level k+1 exists while both extents of level k are even and k < max_mip_level, and each of
its texels is ((p00 + p10) + (p01 + p11)) * 0.25 over its 2 x 2 parents; mip = levels 1 .. nlev-1 one after the other.

Sampling, per slot: empty by texture's rules at level 0 or where any of uv_da = (du/dX, dv/dX, du/dY, dv/dY) is not finite;
ax = dudX Wt, bx = dvdX Ht, sx = ax ax + bx bx, sy likewise, r2 = max(sx, sy); lod = 0 where r2 <= 1, otherwise from r2 = m 2^e,
m in [1, 2) read from the float's bits: lod = 0.5 (e + (m - 1)); lod <= 0: level 0 alone, lod >= nlev - 1: the last level alone,
otherwise j = floor(lod), f = lod - j, out = c_j + f (c_{j+1} - c_j) with c_k texture_ref's bilinear sample of level k.
"""
import numpy as np

import texture_ref as tref

f32 = np.float32
BOUNDARIES = tref.BOUNDARIES
LOD_SHORTFALL = 0.5 * (np.log2(1.0 / np.log(2.0)) - (1.0 / np.log(2.0) - 1.0))       # 0.04304: the most lod falls short of 0.5 log2(r2)


def layout(Ht, Wt, max_mip_level=None):
    """-> (nlev, [(H_k, W_k, offset_k)], T): offset_k = the first texel of level k >= 1 in the packed chain (0 for level 0)."""
    h, w, off, levels = int(Ht), int(Wt), 0, [(int(Ht), int(Wt), 0)]
    while h % 2 == 0 and w % 2 == 0 and (max_mip_level is None or len(levels) - 1 < max_mip_level):
        h, w = h // 2, w // 2
        levels.append((h, w, off))
        off += h * w
    return len(levels), levels, off


def mipmaps(tex, max_mip_level=None, dtype=f32):
    """tex (Ht,Wt,C) or (B,Ht,Wt,C) -> mip (T,C) or (B,T,C) in ``dtype`` (float32: the contract, bit for bit)."""
    tex = np.asarray(tex)
    lead = tex.shape[:-3]
    C = tex.shape[-1]
    nlev, levels, T = layout(tex.shape[-3], tex.shape[-2], max_mip_level)
    cur, parts = tex.astype(dtype), []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, nlev):
            p00, p10 = cur[..., 0::2, 0::2, :], cur[..., 0::2, 1::2, :]
            p01, p11 = cur[..., 1::2, 0::2, :], cur[..., 1::2, 1::2, :]
            cur = (((p00 + p10) + (p01 + p11)) * dtype(0.25)).astype(dtype)
            parts.append(cur.reshape(lead + (-1, C)))
    return np.concatenate(parts, -2) if parts else np.zeros(lead + (0, C), dtype)


def level(tex, mip, k, max_mip_level=None):
    """Level k of the chain as an image (Hk,Wk,C) or (B,Hk,Wk,C): tex itself for k = 0, a view of mip otherwise."""
    tex, mip = np.asarray(tex), np.asarray(mip)
    if k == 0:
        return tex
    _, levels, _ = layout(tex.shape[-3], tex.shape[-2], max_mip_level)
    h, w, off = levels[k]
    return mip[..., off:off + h * w, :].reshape(tex.shape[:-3] + (h, w, tex.shape[-1]))


def mipmaps_backward64(tex_shape, max_mip_level, grad_mip):
    """dL/dtex (tex_shape) float64 for grad_mip of mip's shape: every texel gathers 0.25^k times the gradient of the level-k
    texel above it."""
    Ht, Wt, C = tex_shape[-3:]
    lead = tuple(tex_shape[:-3])
    nlev, levels, T = layout(Ht, Wt, max_mip_level)
    g = np.asarray(grad_mip, np.float64)
    out = np.zeros(lead + (Ht, Wt, C), np.float64)
    jj, ii = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    for k in range(1, nlev):
        h, w, off = levels[k]
        gk = g[..., off:off + h * w, :].reshape(lead + (h, w, C))
        out += 0.25 ** k * gk[..., jj >> k, ii >> k, :]
    return out


def lod32(uv_da, Ht, Wt):
    """-> (lod (..., ) float32 in the contract's operation order, r2 float32).  uv_da (...,4), every component finite."""
    d = np.asarray(uv_da, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        ax, bx = d[..., 0] * f32(Wt), d[..., 1] * f32(Ht)
        ay, by = d[..., 2] * f32(Wt), d[..., 3] * f32(Ht)
        sx, sy = ax * ax + bx * bx, ay * ay + by * by
        r2 = np.maximum(sx, sy).astype(f32)
    bits = np.ascontiguousarray(r2).view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int32) - 127
    m = ((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(f32)
    lod = f32(0.5) * (e.astype(f32) + (m - f32(1.0)))
    return np.where(r2 > f32(1.0), lod, f32(0.0)).astype(f32), r2


def stage(uv, uv_da, Ht, Wt, render_layers=None, max_mip_level=None):
    """The float32 first stage -> dict(empty (B,H,W,L) bool, lod float32, j int (the first level), two bool (a second level
    j + 1 blends in), f float32 (0 where not two), nlev)."""
    nlev, _, _ = layout(Ht, Wt, max_mip_level)
    uv_da = np.asarray(uv_da, f32)
    empty = tref.empty(uv, Ht, Wt, render_layers) | ~np.isfinite(uv_da).all(-1)
    lod, _ = lod32(np.where(empty[..., None], f32(0), uv_da), Ht, Wt)
    low, high = lod <= f32(0), lod >= f32(nlev - 1)
    two = ~empty & ~low & ~high
    jf = np.floor(lod)
    j = np.where(low, 0, np.where(high, nlev - 1, jf.astype(np.int64)))
    f = np.where(two, (lod - jf).astype(f32), f32(0)).astype(f32)
    return dict(empty=empty, lod=np.where(empty, f32(0), lod), j=np.where(empty, 0, j), two=two, f=f, nlev=nlev)


def _ids(st):
    """render_layers for texture_ref's per-level calls: -1 in the slots this op holds empty."""
    return np.where(st["empty"], -1, 0).astype(np.int32)


def forward(uv, uv_da, tex, mip, render_layers=None, boundary_mode="wrap", max_mip_level=None, dtype=f32, st=None, stage_dtype=None):
    """The whole contract: the level of detail in float32, each level's fractions and addresses in ``stage_dtype`` (default:
    ``dtype``), the samples and the blend in ``dtype``.  float32: the contract itself.  float64 with float32 fractions: the
    function grads64 differentiates with respect to tex and mip.  float64 throughout, with a float64 uv and the level of detail
    held fixed through ``st``: that function with exact fractions, for differences in uv below float32's resolution."""
    tex = np.asarray(tex)
    Ht, Wt, C = tex.shape[-3:]
    if st is None:
        st = stage(uv, uv_da, Ht, Wt, render_layers, max_mip_level)
    rl = _ids(st)
    cj = np.zeros(st["j"].shape + (C,), dtype)
    cj1 = np.zeros_like(cj)
    for k in range(st["nlev"]):
        first, second = ~st["empty"] & (st["j"] == k), st["two"] & (st["j"] + 1 == k)
        if not (first.any() or second.any()):
            continue
        lvl = level(tex, mip, k, max_mip_level)
        ck = tref.blend(tref.stage(uv, lvl.shape[-3], lvl.shape[-2], rl, "linear", boundary_mode, stage_dtype or dtype), lvl, "linear", dtype)
        cj = np.where(first[..., None], ck, cj)
        cj1 = np.where(second[..., None], ck, cj1)
    with np.errstate(invalid="ignore", over="ignore"):
        f = st["f"].astype(dtype)[..., None]
        both = (cj + (f * (cj1 - cj).astype(dtype)).astype(dtype)).astype(dtype)
    out = np.where(st["two"][..., None], both, cj)
    return np.where(st["empty"][..., None], dtype(0), out).astype(dtype)


def forward32(uv, uv_da, tex, mip, render_layers=None, boundary_mode="wrap", max_mip_level=None):
    return forward(uv, uv_da, tex, mip, render_layers, boundary_mode, max_mip_level, f32)


def forward64(uv, uv_da, tex, mip, render_layers=None, boundary_mode="wrap", max_mip_level=None, st=None, stage_dtype=None):
    return forward(np.asarray(uv, np.float64 if stage_dtype is None else stage_dtype), uv_da, np.asarray(tex, np.float64),
                   np.asarray(mip, np.float64), render_layers, boundary_mode, max_mip_level, np.float64, st, stage_dtype)


def case(shape, Ht, Wt, seed, max_mip_level=None):
    """Inputs that reach every branch at this texture size -> (uv (B,H,W,L,2), uv_da (B,H,W,L,4), render_layers (B,H,W,L)):
    uv in [-0.5, 1.5]^2 (both borders), footprints from a quarter of a texel (magnified) to four times the coarsest level's
    texel (beyond the last level) with either axis the larger, both signs; one slot in 16 empty by id, one in 32 by a
    non-finite uv, one in 32 by a non-finite uv_da.  ``reach`` counts what came out."""
    rng = np.random.RandomState(seed)
    nlev, _, _ = layout(Ht, Wt, max_mip_level)
    uv = rng.uniform(-0.5, 1.5, shape + (2,)).astype(f32)
    texels = 2.0 ** rng.uniform(-2.0, nlev + 1.0, shape + (2,))             # the footprint's length along X and along Y, in texels
    ang = rng.uniform(0, 2 * np.pi, shape + (2,))
    da = np.stack([texels[..., 0] * np.cos(ang[..., 0]) / Wt, texels[..., 0] * np.sin(ang[..., 0]) / Ht,
                   texels[..., 1] * np.cos(ang[..., 1]) / Wt, texels[..., 1] * np.sin(ang[..., 1]) / Ht], -1).astype(f32)
    rl = np.where(rng.uniform(size=shape) < 1 / 16, -1, rng.randint(0, 50, shape)).astype(np.int32)
    bad = rng.uniform(size=shape)
    uv[bad < 1 / 32, 0] = np.nan
    uv[(bad >= 1 / 32) & (bad < 1 / 24), 1] = np.inf
    da[(bad > 1 - 1 / 32), 2] = -np.inf
    da[(bad > 1 - 1 / 24) & (bad <= 1 - 1 / 32), 1] = np.nan
    return uv, da, rl


def reach(uv, uv_da, Ht, Wt, render_layers=None, max_mip_level=None):
    """dict of slot counts: magnified (lod <= 0), pairs[k] (blended between levels k and k + 1), beyond (0 < lod and lod >=
    nlev - 1: the last level alone), empty_id, empty_uv, empty_da."""
    st = stage(uv, uv_da, Ht, Wt, render_layers, max_mip_level)
    live = ~st["empty"]
    by_id = np.zeros(live.shape, bool) if render_layers is None else np.asarray(render_layers) < 0
    by_uv = tref.empty(uv, Ht, Wt, None)
    by_da = ~np.isfinite(np.asarray(uv_da, f32)).all(-1)
    nlev = st["nlev"]
    return dict(magnified=int((live & (st["lod"] <= 0)).sum()),
                pairs=[int((st["two"] & (st["j"] == k)).sum()) for k in range(nlev - 1)],
                beyond=int((live & ~st["two"] & (st["lod"] >= nlev - 1) & (st["lod"] > 0)).sum()),
                empty_id=int(by_id.sum()), empty_uv=int((by_uv & ~by_id).sum()), empty_da=int((by_da & ~by_id & ~by_uv).sum()))


def grads64(uv, uv_da, tex, mip, render_layers, boundary_mode, max_mip_level, g):
    """(dL/dtex of tex's shape, dL/dmip of mip's shape, dL/duv (B,H,W,L,2)) float64 for upstream g (B,H,W,L,C): lod, j, f, the
    fractions and the addresses from the float32 stage, everything after in float64.  Level k receives texture_ref.grads64 of
    (1 - f) g, f g or g, as the slot weighs it."""
    tex, mip = np.asarray(tex), np.asarray(mip)
    Ht, Wt, C = tex.shape[-3:]
    st = stage(uv, uv_da, Ht, Wt, render_layers, max_mip_level)
    _, levels, _ = layout(Ht, Wt, max_mip_level)
    rl = _ids(st)
    g = np.asarray(g, np.float64)
    f = st["f"].astype(np.float64)
    dtex, dmip = np.zeros(tex.shape, np.float64), np.zeros(mip.shape, np.float64)
    duv = np.zeros(st["j"].shape + (2,), np.float64)
    for k in range(st["nlev"]):
        first, second = ~st["empty"] & (st["j"] == k), st["two"] & (st["j"] + 1 == k)
        m = np.where(first, np.where(st["two"], 1.0 - f, 1.0), 0.0) + np.where(second, f, 0.0)
        if not m.any():
            continue
        dk, du = tref.grads64(uv, level(tex, mip, k, max_mip_level), rl, "linear", boundary_mode, g * m[..., None])
        duv += du
        if k == 0:
            dtex += dk
        else:
            h, w, off = levels[k]
            dmip[..., off:off + h * w, :] += dk.reshape(mip.shape[:-2] + (h * w, C))
    return dtex, dmip, duv
