"""Restatements of the deferred path's ops on a render window (include/dm2_hip.h: dm2_window), built from the full-frame
restatements the tests already have.

A window is (patch_min (B,2) int32, pw, ph): window pixel (x, y) of view b is frame pixel (x + patch_min[b,0], y + patch_min[b,1]).

* rasterize -- the candidates come from the oracle's own binning of the window, ``oracle.cpu.Binning(B, P, F, pw, ph, patch_min,
  ..., key_min_depth=True)`` (tiles anchored at the window's origin), then ``rasterize_ref.hits32`` / ``select`` on the window's
  cut of the rays.
* generate -- the oracle's ``orc_render_layers`` on that binning and those rays.
* coverage, render -- per-pixel ops: the window's layers are embedded into a frame of -1, the full-frame restatement runs, the
  result is cropped.  Exact.

``windows(W, H)`` are the windows the tests share; ``scene2(name)`` the scenes, cut to two views.
"""
import numpy as np

import rasterize_ref as rref

f32 = np.float32
TILE = rref.TILE
SCENES = ("soup", "lattice", "aligned")
_SCENES = {}


def scene2(name):
    """``rasterize_ref.scene`` (soup, lattice) or ``tet_case`` (aligned) with its per-view arrays cut to the first two views."""
    if name not in _SCENES:
        s = dict(rref.tet_case(name) if name in rref.TET_CASES else rref.scene(name))
        for k in ("verts_ndc", "verts_image", "ray_o", "ray_d", "mv", "proj"):
            if k in s:
                s[k] = np.ascontiguousarray(s[k][:2])
        assert s["verts_ndc"].shape[0] == 2
        _SCENES[name] = s
    return _SCENES[name]


def windows(W, H):
    """name -> (patch_min (2,2) int32, pw, ph) in a W x H frame (at least 49 x 49):
      a  the degenerate window: origin 0, the frame's size
      b  origin (16, 16), 32 x 32: origin and size tile-aligned (no partial tile; its tiles are the frame's)
      c  origins (7, 5) and (3, 11), 40 x 33: unaligned, partial tiles on both axes
      d  23 x 19 with the right and bottom edges on the frame's (one origin: the size is shared by the views)
      e  1 x 1 at two different pixels near the centre
      f  empty (pw = 0)"""
    pm = lambda *rows: np.array(rows, np.int32)
    return dict(a=(pm([0, 0], [0, 0]), W, H), b=(pm([16, 16], [16, 16]), 32, 32), c=(pm([7, 5], [3, 11]), 40, 33),
                d=(pm([W - 23, H - 19], [W - 23, H - 19]), 23, 19), e=(pm([W // 2, H // 2], [W // 2 - 5, H // 2 + 3]), 1, 1),
                f=(pm([4, 9], [0, 0]), 0, 13))


def cut(a, pm, pw, ph):
    """The window of a (B,H,W,...) array -> (B,ph,pw,...), a copy."""
    a = np.asarray(a)
    return np.ascontiguousarray(np.stack([a[b, int(y):int(y) + ph, int(x):int(x) + pw] for b, (x, y) in enumerate(np.asarray(pm))]))


def embed(a, pm, W, H, fill):
    """A (B,ph,pw,...) window array inside a (B,H,W,...) frame of ``fill``."""
    a = np.asarray(a)
    out = np.full((a.shape[0], H, W) + a.shape[3:], fill, a.dtype)
    for b, (x, y) in enumerate(np.asarray(pm)):
        out[b, int(y):int(y) + a.shape[1], int(x):int(x) + a.shape[2]] = a[b]
    return out


def binning(s, pm, pw, ph):
    from oracle import cpu as orc
    B, P, F = s["verts_ndc"].shape[0], s["verts"].shape[0], s["faces"].shape[0]
    return orc.Binning(B, P, F, pw, ph, np.ascontiguousarray(pm, np.int32), s["faces"], s["verts_ndc"], s["verts_image"],
                       key_min_depth=True)


def tile_lists(bn):
    """(tiles, J) face ids of the binning's tile lists in list order, -1 behind each list's end."""
    ranges = bn.ranges.astype(np.int64)
    lens = ranges[:, 1] - ranges[:, 0]
    J = int(lens.max()) if lens.size else 0
    jj = np.arange(J)
    valid = jj[None, :] < lens[:, None]
    tl = np.full(valid.shape, -1, np.int64)
    tl[valid] = bn.face_list.astype(np.int64)[(ranges[:, :1] + jj[None, :])[valid]]
    return tl


def candidates(s, pm, pw, ph, face_existence=None):
    """``rasterize_ref.candidates`` for a window: -> (cand (N, J), min_d, max_d), N = B*ph*pw pixels in (b, y, x) order, the
    lists those of the pixel's 16 x 16 WINDOW tile."""
    B, F = s["verts_ndc"].shape[0], s["faces"].shape[0]
    N = B * ph * pw
    if F == 0 or N == 0:
        z = np.zeros((N, 0), f32)
        return np.zeros((N, 0), np.int64), z, z
    gx, gy = (pw + TILE - 1) // TILE, (ph + TILE - 1) // TILE
    bn = binning(s, pm, pw, ph)
    tl = tile_lists(bn)
    if face_existence is not None:
        fe = np.asarray(face_existence, np.int32)
        keep = tl >= 0
        keep[keep] = fe[tl[keep]] != 0
        order = np.argsort(~keep, axis=1, kind="stable")
        tl = np.where(np.take_along_axis(keep, order, 1), np.take_along_axis(tl, order, 1), -1)
        tl = tl[:, :int(keep.sum(1).max())]
    view = (np.arange(tl.shape[0]) // (gx * gy))[:, None]
    fs = np.where(tl >= 0, tl, 0)
    mind = np.where(tl >= 0, bn.min_depths[view * F + fs], f32(0))
    maxd = np.where(tl >= 0, bn.max_depths[view * F + fs], f32(0))
    b, y, x = np.meshgrid(np.arange(B), np.arange(ph), np.arange(pw), indexing="ij")
    tile = ((b * gy + y // TILE) * gx + x // TILE).reshape(-1)
    return tl[tile], mind[tile].astype(f32), maxd[tile].astype(f32)


def rays(s, pm, pw, ph):
    return cut(s["ray_o"], pm, pw, ph), cut(s["ray_d"], pm, pw, ph)


def intersect(s, pm, pw, ph, face_existence=None):
    """``rasterize_ref.intersect`` on the window: its candidates, the window's rays."""
    cand, mind, maxd = candidates(s, pm, pw, ph, face_existence)
    ro, rd = rays(s, pm, pw, ph)
    hit, t, u, v = rref.hits32(s["verts"], s["faces"], cand, ro, rd)
    return dict(shape=(s["verts_ndc"].shape[0], ph, pw), cand=cand, mind=mind, maxd=maxd, hit=hit, t=t, u=u, v=v)


def rasterize32(s, pm, pw, ph, L, face_existence=None):
    return rref.select(intersect(s, pm, pw, ph, face_existence), L)


def generate(ts, ndc, img, ray_o, ray_d, pm, pw, ph, L, existence=None):
    """The oracle's layer generator on a window of tet scene ``ts``: binning of the window, the window's rays (ray_o / ray_d:
    the frame's) -> (layers (B,ph,pw,L), cnt (B,ph,pw))."""
    from oracle import cpu as orc
    c = lambda a, dt: np.ascontiguousarray(np.asarray(a), dtype=dt)
    verts, faces, tets = c(ts.verts, f32), c(ts.faces, np.int32), c(ts.tets, np.int32)
    face_tets, tet_faces = c(ts.face_tets, np.int32), c(ts.tet_faces, np.int32)
    fe = c(ts.faces_existence if existence is None else existence, np.int32)
    ndc, img = c(ndc, f32), c(img, f32)
    B, P, F, T = ndc.shape[0], verts.shape[0], faces.shape[0], tets.shape[0]
    ro, rd = cut(c(ray_o, f32), pm, pw, ph), cut(c(ray_d, f32), pm, pw, ph)
    bn = orc.Binning(B, P, F, pw, ph, c(pm, np.int32), faces, ndc, img, key_min_depth=True)
    layers = np.full((B, ph, pw, L), -1, np.int32); cnt = np.zeros((B, ph, pw), np.int32)
    ff = np.full((B, ph, pw), -1, np.int32); ft = np.full((B, ph, pw), -1, np.int32)
    orc.lib().orc_render_layers(B, P, F, T, pw, ph, orc._p(verts), orc._p(faces), orc._p(tets), orc._p(face_tets), orc._p(tet_faces),
                                orc._p(fe), orc._p(ro), orc._p(rd), bn.handle, L, orc._p(ff), orc._p(ft), orc._p(layers), orc._p(cnt), 1)
    return layers, cnt


def coverage32(layers_win, pm, W, H, verts_image, faces, temperature):
    """``coverage_ref.coverage32`` of the window's layers embedded in a W x H frame of -1 -> (info of the frame, cov of the
    window)."""
    import coverage_ref as cref
    info = cref.coverage32(embed(layers_win, pm, W, H, -1), verts_image, faces, temperature)
    return info, cut(info["cov"], pm, layers_win.shape[2], layers_win.shape[1])


def composite32(inp, pm, W, H):
    """``layer_composite_ref.forward32`` of inputs whose render_layers are a window's and whose ray_o / ray_d the frame's:
    -> (fwd of the frame, dict of the window's color, depth_raw, final_T, n_contrib)."""
    import layer_composite_ref as lref
    rl = np.asarray(inp["render_layers"])
    full = dict(inp, render_layers=embed(rl, pm, W, H, -1))
    fwd = lref.forward32(**full)
    return fwd, {k: cut(fwd[k], pm, rl.shape[2], rl.shape[1]) for k in ("color", "depth_raw", "final_T", "n_contrib")}
