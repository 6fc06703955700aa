"""Structured scenes for the parity tests: pixel-aligned and degenerate geometry.

``scenes.triangle_soup`` draws every vertex from continuous uniforms, so almost no vertex lands on a pixel line, no edge is
axis-parallel or passes through a pixel corner, and no two faces have equal depths.  The scenes here are built to be those
cases: watertight grids on the pixel lattice, sub-pixel triangles on the quarter-pixel lattice, edges with one component
exactly 0 or within a hair of the 1e-3 "iszero" threshold, 4K image coordinates, zero-area faces and coplanar duplicates.

Every generator is a seeded, deterministic function that returns the op's 21 boundary arguments (CPU tensors):
the world geometry is un-projected through ``scenes.camera`` as ``triangle_soup`` does and captured through the package's
own host prep (``util.capture_forward_args``).  For the exact scenes ``verts_image`` (argument 9) is then set to the intended
image coordinates in fp32 and the six AA tables (12-17) are rebuilt from it, CCW reorder included, the way
``util.from_image_oracle_args`` builds them: the materialised-table and the from-image paths see the same geometry.
The ``projected`` scene is not snapped: the prep's own projection puts its vertices within a few ulp of the lattice.
"""
import functools

import numpy as np
import torch

import far
from util import capture_forward_args, scenes


class Layer:
    """Image-space geometry under construction: vertices (px, py) in full-image pixel units, view depth per vertex, faces."""

    def __init__(self):
        self.xy, self.z, self.faces = [], [], []
        self.n = 0

    def add(self, xy, z, faces):
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        self.xy.append(xy)
        self.z.append(np.broadcast_to(np.asarray(z, np.float64), (len(xy),)))
        self.faces.append(np.asarray(faces, np.int64).reshape(-1, 3) + self.n)
        self.n += len(xy)

    def arrays(self):
        return np.concatenate(self.xy), np.concatenate(self.z), np.concatenate(self.faces)


def grid(layer, x0, y0, nx, ny, cell, depth, tilt=0.0):
    """A watertight grid of nx x ny quads of ``cell`` px with its corner at (x0, y0), each quad split along alternating
    diagonals (so that both diagonal directions occur and a vertex is shared by 4 or 8 faces).  ``tilt`` px^-1 adds a depth
    slope along x so that faces of one layer do not all have the same sort key."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    xy = np.stack([x0 + i * cell, y0 + j * cell], -1).reshape(-1, 2).astype(np.float64)
    z = depth + tilt * (xy[:, 0] - x0)
    vid = lambda a, b: b * (nx + 1) + a
    faces = []
    for b in range(ny):
        for a in range(nx):
            p00, p10, p01, p11 = vid(a, b), vid(a + 1, b), vid(a, b + 1), vid(a + 1, b + 1)
            if (a + b) % 2 == 0:
                faces += [(p00, p10, p11), (p00, p11, p01)]
            else:
                faces += [(p00, p10, p01), (p10, p11, p01)]
    layer.add(xy, z, faces)


def _grid_layers(layer, ox=0.0, oy=0.0):
    """Scene 1's geometry (a 56 x 50 frame at offset (ox, oy)): a front layer of four blocks with cells of 1, 2, 3 and 5 px, a
    middle layer of 2 px cells offset by exactly half a pixel (its axis-parallel edges run through pixel centres) and a back
    layer of 3 px cells."""
    grid(layer, ox + 3, oy + 2, 20, 20, 1.0, 2.6, tilt=0.001)
    grid(layer, ox + 27, oy + 2, 10, 10, 2.0, 2.62, tilt=0.001)
    grid(layer, ox + 3, oy + 26, 7, 7, 3.0, 2.64, tilt=0.001)
    grid(layer, ox + 27, oy + 25, 5, 5, 5.0, 2.66)                   # (no tilt: a block of equal sort keys)
    grid(layer, ox - 1.5, oy - 0.5, 30, 26, 2.0, 3.0, tilt=0.002)
    grid(layer, ox - 2, oy - 2, 21, 19, 3.0, 3.4, tilt=0.0005)


def _iszero_faces(layer, rng, n, ox, oy, w, h):
    """Scene 3's faces: one edge with a component of exactly 0, within (0, 1e-3), or just above 1e-3, that touches or
    straddles a pixel line; the third corner a few pixels away.  Half of them along x = const lines, half along y = const."""
    ds = [0.0, 2.5e-4, 6e-4, 9e-4, 9.9e-4, 1.01e-3, 1.1e-3, 1.5e-3]
    for it in range(n):
        d = ds[it % len(ds)] * (1 if (it // len(ds)) % 2 == 0 else -1)
        k = ox + rng.randint(2, w - 2)                                        # the pixel line
        where = it % 3                                                        # start on it / straddling it / end on it
        a0 = k - (0.0 if where == 0 else (d / 2 if where == 1 else d))
        b0 = oy + rng.randint(1, h - 8) + rng.choice([0.0, 0.25, 0.5, rng.uniform(0, 1)])
        L = rng.choice([1.0, 2.0, rng.uniform(1.5, 6.0)])
        side = rng.choice([-1.0, 1.0]) * rng.uniform(1.0, 5.0)
        tri = [(a0, b0), (a0 + d, b0 + L), (a0 + side, b0 + rng.uniform(0, L))]
        if it % 2:                                                            # the transposed case: along a y = const line
            tri = [(b - oy + ox, a - ox + oy) for a, b in tri]
        layer.add(tri, rng.uniform(2.5, 3.5), [(0, 1, 2)])


def _subpixel_faces(layer, rng, n, ox, oy, w, h):
    """Scene 2's faces: 0.25-2 px triangles, every corner on the quarter-pixel lattice (so on pixel lines often)."""
    made = 0
    while made < n:
        a = np.array([ox + rng.randint(-2, 4 * w + 2) / 4.0, oy + rng.randint(-2, 4 * h + 2) / 4.0])
        o = rng.randint(-8, 9, size=(2, 2)) / 4.0
        if abs(o[0, 0] * o[1, 1] - o[0, 1] * o[1, 0]) == 0.0:
            continue
        layer.add([a, a + o[0], a + o[1]], rng.uniform(2.5, 3.5), [(0, 1, 2)])
        made += 1


def _degenerate_faces(layer, rng, n, ox, oy, w, h):
    """Scene 5's faces: zero-area faces (collinear corners along a pixel line and along a diagonal, two coincident corners)
    and faces with a corner exactly on a pixel corner whose opposite edge lies along a pixel line."""
    for it in range(n):
        x, y = ox + rng.randint(3, w - 8), oy + rng.randint(3, h - 8)
        s, t = rng.randint(1, 4), rng.randint(1, 4)
        kind = it % 5
        if kind == 0:
            tri = [(x, y), (x, y + s), (x, y + s + t)]                          # along a pixel line
        elif kind == 1:
            tri = [(x, y), (x + s, y + s), (x + s + t, y + s + t)]              # along a diagonal (through pixel corners)
        elif kind == 2:
            tri = [(x, y), (x, y), (x + s + 0.5, y + t)]                        # two coincident corners
        elif kind == 3:
            tri = [(x + 0.5, y + 0.5), (x + s, y), (x + s + 0.5, y + 0.5)]      # collinear through a pixel centre
        else:
            tri = [(x, y), (x - s, y + t), (x + s + 1, y + t)]                  # corner on a pixel corner, opposite edge on y = y + t
        layer.add(tri, rng.uniform(2.5, 3.2), [(0, 1, 2)])


def _far_faces(layer, rng, n, w, h):
    """Scene "far"'s faces: one or two corners in or next to a pixel of the frame, the others 1e2 to 1e7 px outside it in every
    direction -- tests/far.py's constructions (wedges, slivers, long edges exactly through a pixel corner or a few ulp off it,
    near corners on pixel lines, long nearly axis-parallel edges) around random pixels.  One in eight may cross the frame;
    the others point out of it from near its border (at most 150 of its pixels in the face's bounding box: the pair count of
    bbox_pairs stays small)."""
    made = 0
    while made < n:
        kind = far.KINDS[made % len(far.KINDS)]
        reach = far.REACHES[(made // len(far.KINDS)) % len(far.REACHES)]
        pm = np.array([rng.randint(0, w), rng.randint(0, h)], np.float64)
        tri = far.far_triangle(rng, pm, reach, kind).astype(np.float64)
        lo = np.maximum(np.floor(tri.min(axis=0)), 0); hi = np.minimum(np.floor(tri.max(axis=0)), [w - 1, h - 1])
        if np.prod(np.maximum(hi - lo + 1, 0)) > (w * h if made % 8 == 0 else 150):
            continue
        layer.add(tri, rng.uniform(2.5, 3.5), [(0, 1, 2)])
        made += 1


def _unproject(xy, z, W, H):
    """Image point (px, py) at view depth z -> world point, exactly as scenes.triangle_soup does (fp64, then fp32)."""
    t, aspect = scenes.TAN_HALF_FOV, W / H
    xn = xy[:, 0] / W * 2.0 - 1.0
    yn = xy[:, 1] / H * 2.0 - 1.0
    return np.stack([xn * z * aspect * t, yn * z * t, -z + scenes.CAM_DIST], -1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _geometry(name):
    """-> dict(W, H, xy, z, faces, views = [(patch_min, ...)], pw, ph, nlat) of scene ``name``; fixed seeds."""
    rng = np.random.RandomState(20251015 + sum(map(ord, name)))
    L = Layer()
    W, H, views, pw, ph, nlat = 56, 50, [(0, 0)], None, None, None
    if name in ("grid", "projected"):
        _grid_layers(L)
    elif name == "subpixel":
        W, H = 40, 36
        _subpixel_faces(L, rng, 2400, 0, 0, W, H)
    elif name == "iszero":
        W, H = 48, 40
        _iszero_faces(L, rng, 800, 0, 0, W, H)
        grid(L, -1, -1, 13, 11, 4.0, 3.45)                                   # a backdrop
    elif name == "large":
        # scenes 1 and 3 in a 3840 x 2160 frame, rendered through two patches in two views of one camera
        W, H = 3840, 2160
        _grid_layers(L, 3700, 2000)
        nlat = L.n
        _iszero_faces(L, rng, 400, 3760, 2004, 48, 40)
        views, pw, ph = [(3700, 2000), (3756, 2006)], 56, 44
    elif name == "far":
        # faces through the frame's sides with corners 1e2 .. 1e7 px away, over a backdrop grid
        W, H = 64, 48
        grid(L, -1, -1, 17, 13, 4.0, 3.45)
        nlat = L.n
        _far_faces(L, rng, 300, W, H)
    elif name == "degenerate":
        W, H = 40, 32
        _degenerate_faces(L, rng, 500, 0, 0, W, H)
        grid(L, -1, -1, 11, 9, 4.0, 3.3)
    elif name == "coplanar":
        # a grid repeated at exactly the same depth: once with the same winding, once clockwise (shared vertex rows)
        W, H = 36, 32
        grid(L, 2, 2, 16, 14, 1.0, 2.8)
        grid(L, 1.5, -0.5, 12, 11, 3.0, 3.1)
        xy, z, fc = L.arrays()
        L = Layer()
        L.add(xy, z, np.concatenate([fc, fc, fc[:, [0, 2, 1]]]))
    else:
        raise KeyError(name)
    xy, z, faces = L.arrays()
    # nlat: the leading vertices meant to be on the scene's lattice (LATTICE; all of them where None)
    return dict(W=W, H=H, xy=xy, z=z, faces=faces, views=views, pw=pw or W, ph=ph or H, nlat=len(xy) if nlat is None else nlat)


EXACT = ["grid", "subpixel", "iszero", "large", "degenerate", "coplanar", "far"]
ALL = EXACT + ["projected"]
LATTICE = {"grid": 0.5, "subpixel": 0.25, "large": 0.5, "degenerate": 0.5, "coplanar": 0.5, "projected": 0.5,
           "far": 0.5}   # (None: iszero; far: its backdrop)


def scene(name):
    """The scene as a scenes.SoupScene (one camera per view, all cameras equal) plus its intended image coordinates."""
    g = _geometry(name)
    W, H = g["W"], g["H"]
    B = len(g["views"])
    rng = np.random.RandomState(7 + sum(map(ord, name)))
    verts = torch.from_numpy(_unproject(g["xy"], g["z"], W, H))
    P, F = len(verts), len(g["faces"])
    mv, proj = scenes.camera(W, H)
    sc = scenes.SoupScene(W, H, mv[None].repeat(B, 1, 1), proj[None].repeat(B, 1, 1), verts,
                          torch.from_numpy(g["faces"].astype(np.int32)),
                          torch.from_numpy(rng.uniform(0, 1, (P, 3)).astype(np.float32)),
                          torch.from_numpy(rng.uniform(0.3, 0.9, F).astype(np.float32)),
                          torch.from_numpy(rng.uniform(0.75, 1.25, (B, F)).astype(np.float32)) if B > 1 else torch.ones((1, F)),
                          torch.zeros(3, dtype=torch.float32))
    return sc, g


def snap(args, xy):
    """``args`` with verts_image := ``xy`` in fp32 for every view and the six AA tables rebuilt from it (reorder=True)."""
    from oracle import cpu as orc
    a = list(args)
    B = a[9].shape[0]
    vi = np.ascontiguousarray(np.broadcast_to(xy.astype(np.float32), (B,) + xy.shape))
    fc = a[5].numpy().astype(np.int64)
    F = fc.shape[0]
    with np.errstate(all="ignore"):
        t = orc.aa_tables(vi[:, fc.reshape(-1)].reshape(-1, 3, 2), np.float32, reorder=True)
    a[9] = torch.from_numpy(vi.copy())
    for k, nm in zip(range(12, 17), ("verts", "edges", "iszero", "recip", "normal")):
        a[k] = torch.from_numpy(np.ascontiguousarray(t[nm].reshape(B, F, 3, 2))).to(args[k].dtype)
    a[17] = torch.from_numpy(np.ascontiguousarray(t["normal_c"].reshape(B, F, 3))).to(args[17].dtype)
    return a


@functools.lru_cache(maxsize=None)
def _args(name, temp, K):
    sc, g = scene(name)
    B = len(g["views"])
    args, _ = capture_forward_args(sc, list(range(B)), [list(v) for v in g["views"]], g["pw"], g["ph"], temp, K)
    if name != "projected":
        args = snap(args, g["xy"])
    return tuple(args)


def make_args(name, temp=1.0, K=20):
    """The 21 boundary arguments of scene ``name`` (CPU tensors; a fresh list, the tensors shared between calls)."""
    return list(_args(name, float(temp), int(K)))


def bbox_pairs(args):
    """Every (view, face, pixel) whose pixel lies in the face's image-space bounding box (closed) inside the view's patch:
    -> b, f, pixmin (n, 2) float32 of full-image pixel coordinates."""
    v = args[12].numpy().astype(np.float64)                                   # (B,F,3,2)
    pm = args[1].numpy().astype(np.int64)
    pw, ph = int(args[2]), int(args[3])
    bs, fs, ps = [], [], []
    for b in range(v.shape[0]):
        lo = np.floor(np.nanmin(v[b], axis=1)).astype(np.int64)
        hi = np.floor(np.nanmax(v[b], axis=1)).astype(np.int64)
        lo = np.maximum(lo, pm[b]); hi = np.minimum(hi, pm[b] + [pw - 1, ph - 1])
        for f in np.nonzero((hi >= lo).all(axis=1))[0]:
            xs, ys = np.meshgrid(np.arange(lo[f, 0], hi[f, 0] + 1), np.arange(lo[f, 1], hi[f, 1] + 1))
            ps.append(np.stack([xs.ravel(), ys.ravel()], -1))
            bs.append(np.full(xs.size, b)); fs.append(np.full(xs.size, f))
    return np.concatenate(bs), np.concatenate(fs), np.concatenate(ps).astype(np.float32)


def pair_tables(args, b, f):
    """The six AA tables of the pairs' faces, gathered: dict of numpy arrays (n,3,2) / (n,3)."""
    names = ("verts", "edges", "iszero", "recip", "normal", "normal_c")
    return {nm: np.ascontiguousarray(args[12 + k].numpy()[b, f]) for k, nm in enumerate(names)}


def exact_ties(verts, pixmin):
    """(n) bool: the pair is an exact geometric tie -- a corner of the triangle lies exactly on one of the pixel's four
    boundary lines (within the pixel's extent), or an edge passes exactly through one of the pixel's corners.  fp64 on fp32
    inputs: the differences and products below are exact, the cross product's zero test is too."""
    v = verts.astype(np.float64)                                              # (n,3,2)
    lo = pixmin.astype(np.float64)[:, None, :]; hi = lo + 1.0
    on_x = ((v[..., 0] == lo[..., 0]) | (v[..., 0] == hi[..., 0])) & (v[..., 1] >= lo[..., 1]) & (v[..., 1] <= hi[..., 1])
    on_y = ((v[..., 1] == lo[..., 1]) | (v[..., 1] == hi[..., 1])) & (v[..., 0] >= lo[..., 0]) & (v[..., 0] <= hi[..., 0])
    tie = (on_x | on_y).any(axis=1)
    a, e = v, np.roll(v, -1, axis=1) - v                                      # edges p_i -> p_{i+1}
    for cx, cy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        c = lo[:, 0, :] + [cx, cy]                                            # (n,2)
        d = c[:, None, :] - a
        cross = e[..., 0] * d[..., 1] - e[..., 1] * d[..., 0]
        inseg = (np.minimum(a[..., 0], a[..., 0] + e[..., 0]) <= c[:, None, 0]) & (c[:, None, 0] <= np.maximum(a[..., 0], a[..., 0] + e[..., 0])) \
            & (np.minimum(a[..., 1], a[..., 1] + e[..., 1]) <= c[:, None, 1]) & (c[:, None, 1] <= np.maximum(a[..., 1], a[..., 1] + e[..., 1]))
        tie |= ((cross == 0) & inseg & (np.abs(e).sum(-1) > 0)).any(axis=1)
    return tie


def oracle_pairs(args, b, f, pixmin):
    """The oracle's clipper (oracle.cpu.aa_overlap) on every pair: -> area (n), grad (n,3,2), code (n)."""
    from oracle import cpu as orc
    t = pair_tables(args, b, f)
    n = len(b)
    area = np.zeros(n, np.float32); grad = np.zeros((n, 3, 2), np.float32); code = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            a, g, c = orc.aa_overlap(t, i, pixmin[i], np.float32)
            area[i], code[i] = a, c
            if c == 0:
                grad[i] = g
    return area, grad, code

