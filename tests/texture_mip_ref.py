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


def footprints(rng, shape, Ht, Wt, lo, hi):
    """uv_da with the footprint's length along X and along Y 2^U(lo, hi) texels, at a random angle each."""
    texels = 2.0 ** rng.uniform(lo, hi, shape + (2,))
    ang = rng.uniform(0, 2 * np.pi, shape + (2,))
    return np.stack([texels[..., 0] * np.cos(ang[..., 0]) / Wt, texels[..., 0] * np.sin(ang[..., 0]) / Ht,
                     texels[..., 1] * np.cos(ang[..., 1]) / Wt, texels[..., 1] * np.sin(ang[..., 1]) / Ht], -1).astype(f32)


def case(shape, Ht, Wt, seed, max_mip_level=None):
    """Inputs that reach every branch at this texture size -> (uv (B,H,W,L,2), uv_da (B,H,W,L,4), render_layers (B,H,W,L)):
    uv in [-0.5, 1.5]^2 (both borders), footprints from a quarter of a texel (magnified) to four times the coarsest level's
    texel (beyond the last level) with either axis the larger, both signs; one slot in 16 empty by id, one in 32 by a
    non-finite uv, one in 32 by a non-finite uv_da.  ``reach`` counts what came out."""
    rng = np.random.RandomState(seed)
    nlev, _, _ = layout(Ht, Wt, max_mip_level)
    uv = rng.uniform(-0.5, 1.5, shape + (2,)).astype(f32)
    da = footprints(rng, shape, Ht, Wt, -2.0, nlev + 1.0)
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


def keys(uv, uv_da, Ht, Wt, render_layers=None, boundary_mode="wrap", max_mip_level=None):
    """(B,H,W,L,8) int64: each slot's taps in the kernel's single key space (level 0: j * Wt + i, level k >= 1: Ht * Wt +
    offset_k + j * W_k + i), the first level's four, then the second's; -1 in an empty slot and, where the slot samples one level,
    in the second four."""
    st = stage(uv, uv_da, Ht, Wt, render_layers, max_mip_level)
    _, levels, _ = layout(Ht, Wt, max_mip_level)
    rl = _ids(st)
    out = np.full(st["j"].shape + (8,), -1, np.int64)
    for k, (h, w, off) in enumerate(levels):
        first, second = ~st["empty"] & (st["j"] == k), st["two"] & (st["j"] + 1 == k)
        if not (first.any() or second.any()):
            continue
        idx = tref.stage(uv, h, w, rl, "linear", boundary_mode)["idx"] + (0 if k == 0 else Ht * Wt + off)
        out[..., :4] = np.where(first[..., None], idx, out[..., :4])
        out[..., 4:] = np.where(second[..., None], idx, out[..., 4:])
    return out


def distinct_keys_per_tile(uv, uv_da, Ht, Wt, render_layers=None, boundary_mode="wrap", max_mip_level=None, tile=16, worst=min):
    """The smallest (``worst=max``: the largest) number of distinct keys the slots of one layer address, over the tile x tile
    pixel tiles of every view and over the layers (texture_ref.distinct_texels_per_tile on ``keys``)."""
    ks = keys(uv, uv_da, Ht, Wt, render_layers, boundary_mode, max_mip_level)
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
    """float32 ``a`` moved n floats up (n < 0: down)."""
    a = f32(a)
    for _ in range(abs(n)):
        a = np.nextafter(a, f32(np.inf) if n > 0 else f32(-np.inf))
    return a


def lod_edge_footprints(Ht, Wt, max_mip_level=None):
    """(N,4) float32 uv_da rows on and next to every branch point of the level of detail, by lod32's own arithmetic.  For every
    k in 0 .. nlev: r2 = 4^k exactly (lod = k), on the X axis (2^k / Wt in du/dX) and on the Y axis (2^k / Ht in dv/dY); and,
    searched among the neighbouring floats of that component with a second component of about 2^k 2^-12 or 2^k 2^-11.5 texels
    (whose square is one float of 4^k below it, and one above it), the rows with the nearest r2 below and above 4^k and with the
    nearest lod below and above k.  Then: zeros, +-0 mixes, a denormal, 1e30 (r2 = inf, lod = 64), 3e38 on two components, the Y
    axis the larger and the reverse, negative components."""
    nlev, _, _ = layout(Ht, Wt, max_mip_level)
    rows = []
    for k in range(nlev + 1):
        s = 2.0 ** k
        rows += [[f32(s / Wt), 0, 0, 0], [0, 0, 0, f32(s / Ht)]]
        cand = []
        for i in range(-4, 5):
            a = _step(s / Wt, i)
            for b0 in (0.0, s * 2.0 ** -12 / Ht, s * 2.0 ** -11.5 / Ht):
                for n in ((0,) if b0 == 0.0 else (-1, 0, 1)):
                    cand.append([a, _step(b0, n), 0, 0])
        cand = np.array(cand, f32)
        lod, r2 = lod32(cand, Ht, Wt)
        if k == 0:
            lod = np.where(r2 < 1, f32(-1), lod)              # (below r2 = 1 every lod is 0: rank those rows by r2 alone)
        exact = cand[r2 == f32(4.0 ** k)]
        assert len(exact), (Ht, Wt, k)
        for val, ref in ((r2, f32(4.0 ** k)), (lod, f32(k))):
            lo, hi = val < ref, val > ref
            if lo.any():
                rows.append(cand[lo][np.argmax(val[lo])])
            if hi.any():
                rows.append(cand[hi][np.argmin(val[hi])])
    z, n0 = f32(0.0), f32(-0.0)
    rows += [[z, z, z, z], [z, n0, z, n0], [n0, z, n0, z], [n0, n0, n0, n0], [1e-45, 0, 0, -1e-45], [1e30, 0, 0, 0], [0, 0, 0, -1e30],
             [3e38, 3e38, 0, 0], [0, 0, -3e38, 3e38], [1.0 / Wt, 0, 0, 3.0 / Ht], [3.0 / Wt, 0, 0, 1.0 / Ht],
             [-2.0 / Wt, -1.0 / Ht, 0.5 / Wt, -0.25 / Ht], [-0.25 / Wt, 0.5 / Ht, -3.0 / Wt, -2.0 / Ht]]
    table = np.array(rows, f32)
    _, first = np.unique(table.view(np.uint32), axis=0, return_index=True)              # by bits: -0.0 is not 0.0
    return table[np.sort(first)]


# ---- the input sets of the GPU tests beyond ``case`` (tests/test_texture_mip_cpu.py holds each to the condition it is for) ----

OVERFLOW_SHAPE, OVERFLOW_SIZE = (2, 32, 48, 2), (512, 512)
HOT_SHAPE = (2, 50, 70, 4)
EDGE_SHAPE = (1, 16, 16, 2)
EDGE_TEXTURES = (((16, 8), None), ((8, 8), None), ((6, 10), None), ((16, 8), 1))        # (Ht, Wt), max_mip_level
LATTICE_SHAPE, LATTICE_SIZE = (1, 33, 47, 2), (16, 8)
LATTICE_SCALES = (0.5, 1.0, 2.0, 4.0, 16.0)        # uv_da = (s / Wt, s / Ht, 0, 0): r2 = 2 s^2, lod = 0, 0.5, 1.5, 2.5 and 4.5 (beyond)


def overflow_case():
    """Random uv in [0, 1)^2 on a 512^2 texture, footprints of 2^U(-1, 3.5) texels: every tile addresses several times the
    keys the scatter's table holds, over levels 0 .. 5 -> (uv, uv_da, render_layers with -1 in one slot of seven)."""
    rng = np.random.RandomState(51)
    uv = rng.uniform(0.0, 1.0, OVERFLOW_SHAPE + (2,)).astype(f32)
    da = footprints(rng, OVERFLOW_SHAPE, *OVERFLOW_SIZE, -1.0, 3.5)
    return uv, da, rng.randint(-1, 6, OVERFLOW_SHAPE).astype(np.int32)


def hot_case_magnified():
    """Every slot magnified into one corner of an (8, 8) texture: a tile's lanes share a handful of level-0 keys."""
    rng = np.random.RandomState(52)
    uv = rng.uniform(0.32, 0.48, HOT_SHAPE + (2,)).astype(f32)
    return uv, footprints(rng, HOT_SHAPE, 8, 8, -4.0, -0.5)


def hot_case_beyond(Ht, Wt):
    """Every footprint at least four times the coarsest level's texel, one slot in eight at 1e30 (r2 = inf): every tap of every
    slot on the top level's texels."""
    rng = np.random.RandomState(53)
    nlev, _, _ = layout(Ht, Wt)
    uv = rng.uniform(-0.5, 1.5, HOT_SHAPE + (2,)).astype(f32)
    da = footprints(rng, HOT_SHAPE, Ht, Wt, nlev + 1.0, nlev + 6.0)
    huge = rng.uniform(size=HOT_SHAPE) < 1 / 8
    da[huge] = 0
    da[huge, rng.randint(0, 4, int(huge.sum()))] = 1e30
    return uv, da


def lod_edge_case(Ht, Wt, max_mip_level=None):
    """``lod_edge_footprints`` tiled over EDGE_SHAPE, uv random in [-0.5, 1.5]^2."""
    rng = np.random.RandomState(54 + Ht + Wt)
    table = lod_edge_footprints(Ht, Wt, max_mip_level)
    n = int(np.prod(EDGE_SHAPE))
    assert len(table) <= n // 4
    da = table[np.arange(n) % len(table)].reshape(EDGE_SHAPE + (4,))
    return rng.uniform(-0.5, 1.5, EDGE_SHAPE + (2,)).astype(f32), np.ascontiguousarray(da)


def lattice_case(scale, outside=False):
    """uv from the lattice {k / 32 : k = -40 .. 72} on both axes (``outside``: k <= 0 or k >= 32 only: under clamp every tap of
    every level beyond the border), one footprint for all slots: uv_da = (scale / Wt, scale / Ht, 0, 0)."""
    rng = np.random.RandomState(55)
    ks = np.arange(-40, 73)
    if outside:
        ks = ks[(ks <= 0) | (ks >= 32)]
    uv = (ks[rng.randint(0, len(ks), LATTICE_SHAPE + (2,))] / 32.0).astype(f32)
    Ht, Wt = LATTICE_SIZE
    da = np.broadcast_to(np.array([scale / Wt, scale / Ht, 0, 0], f32), LATTICE_SHAPE + (4,)).copy()
    return uv, da


# u (v) at which level 0's x = u * Wt - 0.5 (y) meets the range rule on LATTICE_SIZE.  Between 2^23 and 2^24 the product p is a
# whole number and p - 0.5 a tie that rounds to the even neighbour, so x = 2^24 - 1 cannot come out: p = 2^24 - 1 gives 2^24 - 2,
# the largest x a slot can have, and its negation gives -2^24.  (value, live)
RANGE_EDGES = ((2.0 ** 24 - 1, True), (2.0 ** 24, False), (-(2.0 ** 24 - 1), False), (-(2.0 ** 24), False), (-(2.0 ** 24 - 2), True))


def range_case(uv):
    """``uv`` with the RANGE_EDGES products on u in the first ten slots of row 0 and on v in those of row 1 (both layers of five
    pixels each) -> (uv, live (10,) bool in slot order)."""
    uv = uv.copy()
    Ht, Wt = LATTICE_SIZE
    live = []
    for n, (p, ok) in enumerate(RANGE_EDGES * 2):
        uv[0, 0, n // 2, n % 2, 0] = f32(p / Wt)
        uv[0, 1, n // 2, n % 2, 1] = f32(p / Ht)
        live.append(ok)
    return uv, np.array(live)


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


INST_TEXTURE = (8, 4)                     # (Ht, Wt): three levels


def instantiation_case(seed=0):
    """The "every instantiation once" inputs (texture_ref.INST_SHAPE, texture_ref.instantiation_ids) for INST_TEXTURE ->
    (uv, uv_da, render_layers): uv in [-0.5, 1.5]^2, footprints from a quarter of a texel to four times the coarsest level's
    texel, so that lod <= 0, between two levels, and at or above the top level all occur; a few NaN / infinite uv and uv_da."""
    rl = tref.instantiation_ids(seed)
    rng = np.random.default_rng(seed + 3)
    uv = rng.uniform(-0.5, 1.5, tref.INST_SHAPE + (2,)).astype(f32)
    da = footprints(rng, tref.INST_SHAPE, *INST_TEXTURE, -2.0, 4.0)
    tref.spoil(uv, rl, seed)
    tref.spoil(da, rl, seed + 10, n=4)
    return uv, da, rl
