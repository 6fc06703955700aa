"""The windowed restatements (tests/window_ref.py) against the full-frame ones, without a GPU: what a render window of
Renderer.rasterize must and need not share with the crop of the full frame, and that the shared windows reach what the GPU
tests rely on (tiles with several candidates, partial tiles)."""
import numpy as np
import pytest

import rasterize_ref as rref
import window_ref as wref

OUTS = ("layers", "cnt", "bary", "t")
LS = (1, 4, 17)
_FULL = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _full(name):
    """The full-frame restatement's intersections of a scene, computed once."""
    if name not in _FULL:
        s = wref.scene2(name)
        _FULL[name] = rref.intersect(s["W"], s["H"], s["verts"], s["faces"], None, s["verts_ndc"], s["verts_image"], s["ray_o"],
                                     s["ray_d"])
    return _FULL[name]


@pytest.mark.parametrize("name", wref.SCENES)
@pytest.mark.parametrize("win", ["a", "b"])
def test_aligned_windows_are_crops(name, win):
    """(a) the degenerate window and (b) a tile-aligned one: the window's tiles are tiles of the frame, so every array equals the
    crop of the full-frame restatement, bit for bit."""
    s = wref.scene2(name)
    pm, pw, ph = wref.windows(s["W"], s["H"])[win]
    x = wref.intersect(s, pm, pw, ph)
    for L in LS:
        got, full = rref.select(x, L), rref.select(_full(name), L)
        for k in OUTS:
            want = wref.cut(full[k], pm, pw, ph)
            assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
            assert np.array_equal(_bits(got[k]), _bits(want)), (name, win, L, k)
        assert got["cnt"].sum() > 0


def _hit_sets(x):
    """Per pixel the set of faces that are hits among its candidates."""
    return [set(x["cand"][p][x["hit"][p]].tolist()) for p in range(x["hit"].shape[0])]


@pytest.mark.parametrize("name", wref.SCENES)
def test_unaligned_window_differs_only_through_the_tile_grid(name):
    """(c): the window's tiles straddle the frame's.  A face is a candidate of a pixel when its bbox touches the pixel's tile, so
    a face can be listed under one grid and not the other.  Wherever a slot of the window differs from the crop of the full
    frame, the pixel has a hit whose face, as the oracle bins it, is in the pixel's tile list in one grid and not in the other --
    and the first differing slot holds such a face on one of the two sides.  Pixels without such a hit agree in every array."""
    s = wref.scene2(name)
    pm, pw, ph = wref.windows(s["W"], s["H"])["c"]
    xw = wref.intersect(s, pm, pw, ph)
    xf = _full(name)
    B, H, W = xf["shape"]
    # the frame's per-pixel rows, cut to the window (row p of the window <-> its frame pixel)
    idx = wref.cut(np.arange(B * H * W).reshape(B, H, W), pm, pw, ph).reshape(-1)
    cand_f, hit_f = xf["cand"][idx], xf["hit"][idx]
    hw = _hit_sets(xw)
    hf = _hit_sets(dict(cand=cand_f, hit=hit_f))
    lw = [set(r[r >= 0].tolist()) for r in xw["cand"]]
    lf = [set(r[r >= 0].tolist()) for r in cand_f]
    odd = np.zeros(len(hw), bool)
    for p, (a, b) in enumerate(zip(hw, hf)):
        only_w, only_f = a - b, b - a
        assert not (only_w & lf[p]) and not (only_f & lw[p]), (name, p)     # (the same ray decides alike: the lists differ)
        odd[p] = bool(only_w or only_f)
    n_slots = 0
    for L in LS:
        got, full = rref.select(xw, L), rref.select(xf, L)
        want = {k: wref.cut(full[k], pm, pw, ph) for k in OUTS}
        diff = np.zeros(len(hw), bool)
        for k in OUTS:
            d = _bits(got[k]) != _bits(want[k])
            diff |= d.reshape(len(hw), -1).any(1)
        assert not (diff & ~odd).any(), (name, L)
        gl, wl = got["layers"].reshape(len(hw), L), want["layers"].reshape(len(hw), L)
        for p in np.nonzero(diff)[0]:
            k = int(np.nonzero(gl[p] != wl[p])[0][0]) if (gl[p] != wl[p]).any() else None
            assert k is not None, (name, L, p)                                # (ids agree -> the same hits -> the same bits)
            sym = hw[p] ^ hf[p]
            assert int(gl[p, k]) in sym or int(wl[p, k]) in sym, (name, L, p, k)
        n_slots += int((got["layers"] != want["layers"]).sum())
    print(f"{name}, window c: {int(odd.sum())} of {len(hw)} pixels have a hit listed under one grid only; "
          f"{n_slots} differing slots over L = {LS}")


@pytest.mark.parametrize("name", wref.SCENES)
def test_windows_reach_crowded_and_partial_tiles(name):
    """Every non-empty window bins more than one candidate into some tile, and every window whose size is no multiple of 16 has
    a partial tile with candidates ((b) is tile-aligned by construction: it has none); the empty window has no pixel."""
    s = wref.scene2(name)
    for win, (pm, pw, ph) in wref.windows(s["W"], s["H"]).items():
        if win == "f":
            assert pw * ph == 0 and wref.candidates(s, pm, pw, ph)[0].shape[0] == 0
            continue
        bn = wref.binning(s, pm, pw, ph)
        lens = (bn.ranges[:, 1].astype(np.int64) - bn.ranges[:, 0]).reshape(2, bn.gy, bn.gx)
        assert lens.max() > 1, (name, win)
        partial = np.zeros((bn.gy, bn.gx), bool)
        if pw % 16:
            partial[:, -1] = True
        if ph % 16:
            partial[-1, :] = True
        if win == "b":
            assert not partial.any()
        else:
            assert partial.any() and (lens[:, partial] > 1).any(), (name, win)
        if win == "c":
            assert partial[-1, -1] and partial[0, -1] and partial[-1, 0]       # partial on both axes
        x = wref.intersect(s, pm, pw, ph)
        assert x["hit"].any(), (name, win)


def test_embed_and_cut_are_inverse():
    rng = np.random.RandomState(0)
    pm, pw, ph = wref.windows(65, 49)["c"]
    a = rng.randint(0, 9, (2, ph, pw, 3)).astype(np.int32)
    e = wref.embed(a, pm, 65, 49, -1)
    assert np.array_equal(wref.cut(e, pm, pw, ph), a)
    assert (e == -1).sum() == e.size - a.size + (a == -1).sum()
