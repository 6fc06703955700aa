"""Scenes for the default backward's tie path (tests/test_gpu_tie_queue.py): how many ties a tile's chunks carry decides which
way they travel -- through the block's 64-entry LDS buffer, drained at 32 entries and emptied in the tile's last chunk, or,
once a chunk has filled the buffer, straight to the global queue.

Lattice geometry (structured.Layer / structured.grid, see lattice(): ties of the polygon-free Jacobian that carry gradient) and
slivers along pixel rows (a row of ties per face) are mixed with generic soup faces (scenes.triangle_soup: hardly any ties) to set that number.  The
lattice vertices are snapped to their intended image coordinates (structured.snap); the soup's keep what the host prep projects.
Nothing here calls the GPU; every generator is a seeded, deterministic function that returns the op's 21 boundary arguments."""
import functools

import numpy as np
import torch

import structured as S
from util import capture_forward_args, scenes


def _soup(W, H, F, seed, depth_complexity):
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + seed, depth_complexity=depth_complexity)
    return sc.verts.numpy(), sc.faces.numpy().astype(np.int64), sc.verts_color.numpy(), sc.faces_opacity.numpy()


def build(W, H, layer=None, soup=None, views=((0, 0),), pw=None, ph=None, temp=1.0, K=20, seed=0):
    """``layer``: a structured.Layer in full-image pixels (or None); ``soup``: (faces, seed, depth complexity) of a
    scenes.triangle_soup over the same frame (or None); ``views``: one patch_min per view, all views through one camera."""
    rng = np.random.RandomState(977 + seed)
    verts, faces, colors, opac = [], [], [], []
    nlat, xy = 0, None
    if layer is not None:
        xy, z, fc = layer.arrays()
        nlat = len(xy)
        verts.append(S._unproject(xy, z, W, H)); faces.append(fc)
        colors.append(rng.uniform(0, 1, (nlat, 3)).astype(np.float32))
        opac.append(rng.uniform(0.3, 0.9, len(fc)).astype(np.float32))
    if soup is not None:
        v, fc, c, o = _soup(W, H, *soup)
        verts.append(v); faces.append(fc + nlat); colors.append(c); opac.append(o)
    verts, faces = np.concatenate(verts), np.concatenate(faces)
    B, F = len(views), len(faces)
    mv, proj = scenes.camera(W, H)
    intense = rng.uniform(0.75, 1.25, (B, F)).astype(np.float32) if B > 1 else np.ones((1, F), np.float32)
    sc = scenes.SoupScene(W, H, mv[None].repeat(B, 1, 1), proj[None].repeat(B, 1, 1), torch.from_numpy(verts),
                          torch.from_numpy(faces.astype(np.int32)), torch.from_numpy(np.concatenate(colors)),
                          torch.from_numpy(np.concatenate(opac)), torch.from_numpy(intense), torch.zeros(3, dtype=torch.float32))
    args, _ = capture_forward_args(sc, list(range(B)), [list(v) for v in views], pw or W, ph or H, temp, K)
    if nlat:
        vi = args[9][0].numpy().astype(np.float64).copy()                     # (one camera: every view has the same)
        vi[:nlat] = xy
        args = S.snap(args, vi)
    return list(args)


OY = 0.25                              # the lattices' offset along y (see lattice)


def lattice(layer, x0, y0, nx, ny, cw, ch, depth, tilt=0.0):
    """structured.grid with cells of cw x ch px.  The scenes here put its corner at (integer, integer + 1/4) with cells of
    2 x 1 or 4 x 2 px: every vertex lies on a vertical pixel line and every second edge along one, so the pairs are exact ties,
    and the faces cover their pixels in part, so the ties carry gradient.  Vertices on pixel CORNERS will not do: the
    reference's clipper gives an error code to most pairs whose pixel corner an edge runs through, which are never blended,
    and what is left are the pixels a face covers whole, whose area has no gradient (a grid of 1-px square cells blends
    nothing at all: both diagonals run through the pixel's centre)."""
    tmp = S.Layer()
    S.grid(tmp, 0, 0, nx, ny, 1.0, 0.0)
    xy, _, fc = tmp.arrays()
    xy = xy * [cw, ch] + [x0, y0]
    layer.add(xy, depth + tilt * (xy[:, 0] - x0), fc)


def _interleave(layer, x0, y0, nx, ny, cw, ch, depths, keep=1):
    """Lattice triangles one by one (no shared vertices), face i at its own depth depths[i % len]: the depth sort then spreads
    a grid's faces over the list instead of keeping a layer together.  ``keep``: every keep-th face of the grid."""
    tmp = S.Layer()
    lattice(tmp, x0, y0, nx, ny, cw, ch, 0.0)
    xy, _, fc = tmp.arrays()
    for i, f in enumerate(fc[::keep]):
        layer.add(xy[f], depths[i % len(depths)], [(0, 1, 2)])


def slivers(layer, x0, x1, rows, depth, height=1.6):
    """One face per pixel row k of ``rows``, from x0 to x1, whose lower edge runs a hair inside the row, from y = k + 0.003 to
    k + 0.007: nearly axis-parallel (|e.y| < 1/64, yet above the reference's 1e-3 "iszero" threshold) with its ends within 1/64 of
    the pixel line y = k, so every pixel of the row that the face covers is a tie, and is covered in part: x1 - x0 ties with
    gradient per face, where a lattice face gives one or two."""
    for i, k in enumerate(rows):
        layer.add([(x0, k + 0.003), (x1, k + 0.007), (0.5 * (x0 + x1) + 0.37, k + height)], depth + 0.004 * i, [(0, 1, 2)])


def direct():
    """One 16x16 frame, two depth layers of a lattice grid and, between them, three of slivers: a chunk's 256 pairs hold more
    ties than the buffer."""
    L = S.Layer()
    lattice(L, -2, OY - 1, 10, 18, 2.0, 1.0, 2.7, tilt=0.001)
    for k in range(3):
        slivers(L, -1.3 - k, 17.2 + k, range(0, 15), 2.8 + 0.1 * k)
    lattice(L, -2, OY - 1, 10, 18, 2.0, 1.0, 3.2, tilt=0.001)
    return build(16, 16, L, seed=1)


def tail():
    """48x32 of generic soup faces plus three lattice triangles in one tile: a handful of ties, all of them leave with their
    tile's last chunk."""
    L = S.Layer()
    L.add([(20, 4 + OY), (22, 4 + OY), (22, 5 + OY)], 2.8, [(0, 1, 2)])
    L.add([(26, 8 + OY), (28, 9 + OY), (26, 9 + OY)], 3.0, [(0, 1, 2)])
    L.add([(18, 10 + OY), (20, 10 + OY), (20, 11 + OY)], 3.2, [(0, 1, 2)])
    return build(48, 32, L, soup=(24, 11, 2.0), seed=2)


THRESHOLD_KEEP = 2                     # every second face of each lattice layer
THRESHOLD_SOUP = (400, 12, 12.0)       # soup faces, seed, depth complexity


def threshold():
    """16x16: a lattice grid of 2 x 1 px cells in three depth layers, its faces spread in depth between soup faces, so that the tile's ties
    come a few per chunk: the buffer passes 32 entries several times and never fills."""
    L = S.Layer()
    rng = np.random.RandomState(5)
    for k in range(3):
        _interleave(L, 0, OY - 1, 8, 17, 2.0, 1.0, rng.uniform(2.55, 3.45, 97), keep=THRESHOLD_KEEP)
    return build(16, 16, L, soup=THRESHOLD_SOUP, seed=3)


def windows():
    """The lattice scene of the views-and-windows case: a 64x48 frame, a grid of 2 x 1 px cells in front of one of 4 x 2 px
    cells, both with shared vertices, and slivers behind them, seen through two 32x32 windows with different patch_min."""
    L = S.Layer()
    lattice(L, 4, 4 + OY, 20, 36, 2.0, 1.0, 2.6, tilt=0.001)
    lattice(L, 0, OY - 2, 16, 25, 4.0, 2.0, 3.0, tilt=0.002)
    slivers(L, -1.3, 65.2, range(1, 47, 2), 3.3, height=1.2)
    return build(64, 48, L, views=((0, 0), (24, 12)), pw=32, ph=32, seed=4)


def none():
    """A soup frame without a tie: a few large generic faces."""
    return build(32, 32, None, soup=(12, 13, 3.0), seed=5)


SCENES = {"direct": direct, "tail": tail, "threshold": threshold, "windows": windows, "none": none}


@functools.lru_cache(maxsize=None)
def _args(name):
    return tuple(SCENES[name]())


def make_args(name):
    """The 21 boundary arguments of scene ``name`` (CPU tensors; a fresh list, the tensors shared between calls)."""
    return list(_args(name))
