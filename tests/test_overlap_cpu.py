"""The restatement of rasterize's overlap mode (tests/overlap_ref.py) held to float64 and to the restatements it stands on,
and the scenes of tests/test_gpu_overlap.py shown to reach what they are for.  No GPU."""
import numpy as np
import pytest
import torch

import coverage_ref as cref
import overlap_ref as oref
import rasterize_ref as rref
import window_ref as wref
from util import GRAD_TOL, rel_linf, table_capacity

f32 = np.float32
L_ALL = 12             # long enough that almost no list of the small scenes is truncated


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_grads64_against_central_differences_on_every_clamp_code():
    """``grads64`` (autograd with the float32 clamp codes held fixed) against float64 central differences of the same loss, on
    slots of every clamp code 0..6 of the soup: per code up to eight slots, each alone in a list of its own."""
    s = oref.scene("soup")
    r = oref.select(oref.evaluated("soup"), 4)
    codes = oref.slot_codes(s["verts"], s["faces"], r["layers"], s["ray_o"], s["ray_d"])
    assert np.array_equal(codes == 0, r["inside"]) and np.array_equal(codes >= 0, r["layers"] >= 0)
    rng = np.random.default_rng(5)
    rl = np.full_like(r["layers"], -1)
    for c in range(7):
        idx = np.argwhere(codes == c)
        assert len(idx), f"no slot of clamp code {c}"
        for i in idx[rng.permutation(len(idx))[:8]]:
            rl[tuple(i)] = r["layers"][tuple(i)]
    kept = oref.slot_codes(s["verts"], s["faces"], rl, s["ray_o"], s["ray_d"])
    print("slots per code:", np.bincount(kept[kept >= 0], minlength=7))
    gb = rng.standard_normal(rl.shape + (3,))
    gt = rng.standard_normal(rl.shape)
    got = oref.grads64(s["verts"], s["faces"], rl, s["ray_o"], s["ray_d"], gb, gt)

    m = rl >= 0
    pix = np.nonzero(m)
    ro = torch.as_tensor(s["ray_o"].astype(np.float64)[pix[:3]])
    rd = torch.as_tensor(s["ray_d"].astype(np.float64)[pix[:3]])
    vid = s["faces"].astype(np.int64)[rl[m]]
    code = kept[m]
    gbm, gtm = torch.as_tensor(gb[m]), torch.as_tensor(gt[m])

    def loss(v):
        v = torch.as_tensor(v)
        b, t = oref.slot_values64(ro, rd, v[vid[:, 0]], v[vid[:, 1]], v[vid[:, 2]], code)
        return float(((gbm * b).sum(-1) + gtm * t).sum())

    v0 = s["verts"].astype(np.float64)
    want = np.zeros_like(v0)
    h = 1e-6
    for p in np.unique(vid):
        for k in range(3):
            a, b = v0.copy(), v0.copy()
            a[p, k] += h; b[p, k] -= h
            want[p, k] = (loss(a) - loss(b)) / (2 * h)
    assert np.abs(want).max() > 0
    print("grads64 vs central differences:", rel_linf(got, want))
    assert rel_linf(got, want) <= 1e-6
    # per code: the slots of that code alone
    for c in range(7):
        only = np.where(kept == c, rl, -1)
        g = oref.grads64(s["verts"], s["faces"], only, s["ray_o"], s["ray_d"], gb, gt)
        if c in (1, 2, 3):
            assert np.abs(oref.grads64(s["verts"], s["faces"], only, s["ray_o"], s["ray_d"], gb, None)).max() == 0   # bary is a constant corner
        assert np.abs(g).max() > 0, c


def test_projected_t_is_continuous_across_the_edge():
    """On the triangle's edge the clamped point is the hit: the projection formula gives the intersection's t (float64)."""
    rng = np.random.default_rng(2)
    p = torch.as_tensor(rng.standard_normal((50, 3, 3)) + np.array([0, 0, -4.0]))
    w = rng.uniform(0.1, 0.9, 50)
    hit = torch.as_tensor(w[:, None]) * p[:, 0] + torch.as_tensor(1 - w[:, None]) * p[:, 1]      # on edge p0 p1: v = 0
    ro = torch.zeros(50, 3, dtype=torch.float64)
    rd = hit / hit.norm(dim=-1, keepdim=True)
    for code in (0, 5):
        _, t = oref.slot_values64(ro, rd, p[:, 0], p[:, 1], p[:, 2], np.full(50, code))
        assert torch.allclose(t, hit.norm(dim=-1), rtol=1e-12, atol=1e-12), code


CASES = [(n, None) for n in oref.SCENES] + [("soup", "c"), ("aligned", "d"), ("crowded", "crowded"), ("staircase", None)]


@pytest.mark.parametrize("name,win", CASES)
def test_scenes_list_off_triangle_slots_and_inside_slots_are_the_standard_hits(name, win):
    """On every scene of the GPU tests: slots with inside false and area > 0 exist; every listed slot has a non-zero
    ``coverage_ref.coverage32`` at temperature 1; the inside slots are, in order and bit for bit, hits of the standard selection,
    and a standard hit that the overlap lists lack is one the clipper gives no area for (an error or area 0)."""
    s = oref.scene(name)
    pm, pw, ph = oref.window_of(name, win)
    L = L_ALL if name != "crowded" else 40
    for exist in ((False, True) if name in ("soup", "lattice") else (name == "crowded",)):
        x = oref.evaluated(name, win, exist)
        r = oref.select(x, L)
        have = r["layers"] >= 0
        off = have & ~r["inside"]
        assert off.any() and (r["area"][off] > 0).all() and (r["area"][have] > 0).all()
        info, cov = wref.coverage32(r["layers"], pm, s["W"], s["H"], s["verts_image"], s["faces"], 1.0)
        assert (cov[have] != 0).all() and np.array_equal(_bits(cov[have]), _bits(r["area"][have]))      # (1 - 1) + area * 1
        std = rref.select(wref.intersect(s, pm, pw, ph, s["fe"] if exist else None), L)
        full = (r["cnt"] == L) | (std["cnt"] == L)                              # a truncated list: nothing is claimed there
        missing = 0
        for b, y, xx in np.argwhere(~full):
            ins = r["inside"][b, y, xx]
            ids = r["layers"][b, y, xx][ins]
            sid = std["layers"][b, y, xx][:std["cnt"][b, y, xx]]
            keep = np.isin(sid, ids)
            assert np.array_equal(sid[keep], ids), (name, b, y, xx, sid, ids)                          # a subset, in order
            assert np.array_equal(_bits(std["bary"][b, y, xx][:len(sid)][keep]), _bits(r["bary"][b, y, xx][ins]))
            assert np.array_equal(_bits(std["t"][b, y, xx][:len(sid)][keep]), _bits(r["t"][b, y, xx][ins]))
            for f in sid[~keep]:                                                # a hit without an area: the clipper's word
                j = np.nonzero(x["cand"][(b * ph + y) * pw + xx] == f)[0][0]
                n = (b * ph + y) * pw + xx
                assert not x["listed"][n, j] and x["code"][n, j] == 0 and (x["err"][n, j] != 0 or x["area"][n, j] == 0), (name, b, y, xx, f)
                missing += 1
        print(f"{name} win={win} exist={exist}: {int(have.sum())} slots, {int(off.sum())} off-triangle, "
              f"{int(full.sum())} pixels with a full list, {missing} standard hits the clipper gives no area")
        assert (~full).sum() > 0.5 * full.size or name == "crowded"


def test_crowded_scene_reaches_chunks_and_the_table_overflow():
    x = oref.evaluated("crowded", "crowded", False)
    assert (x["cand"] >= 0).sum(1).min() > 256                                   # several LDS chunks in every tile
    r = oref.select(x, 8)
    pm, pw, ph = oref.CROWDED_WINDOW
    counts = [len(np.unique(t[t >= 0])) for b in range(2) for ty in range(0, ph, 16) for tx in range(0, pw, 16)
              for t in [r["layers"][b, ty:ty + 16, tx:tx + 16]]]
    print("crowded: distinct listed faces per window tile at L = 8:", counts, "table", table_capacity())
    assert min(counts) > table_capacity()


def test_coverage_mask_restatement():
    """A slot with inside == 0 gets area * temperature, 0 at temperature 0; the others coverage_ref's value."""
    s = oref.scene("soup")
    r = oref.select(oref.evaluated("soup"), 4)
    for temp in cref.TEMPERATURES:
        cov, info = oref.coverage32(r["layers"], r["inside"], s["verts_image"], s["faces"], temp)
        have = r["layers"] >= 0
        off = have & ~r["inside"]
        assert np.array_equal(_bits(cov[~off]), _bits(info["cov"][~off]))
        assert np.array_equal(_bits(cov[off]), _bits((info["area"][off] * f32(temp)).astype(f32)))
        assert (cov[off] > 0).all() if temp > 0 else (cov[off] == 0).all()


# ---- the equivalence scene -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [None, "patch"])
def test_staircase_lists_nothing_ambiguous(win):
    """Forward's tile-list order and the (t, id) order agree at every pixel of the staircase scene, no exception; with STAIR_L
    slots the last one is empty everywhere (nothing truncated)."""
    s = oref.scene("staircase")
    w = None if win is None else oref.STAIR_PATCH
    x = oref.evaluate(s, w)
    good = oref.list_order_agrees(s, x, w)
    assert good.all(), int((~good).sum())
    r = oref.select(x, oref.STAIR_L)
    assert (r["layers"][..., -1] == -1).all() and r["cnt"].max() >= 4
    assert ((r["layers"] >= 0) & ~r["inside"]).any(-1).sum() > 0.2 * good.size       # silhouette pixels: what the scene is for


@pytest.mark.parametrize("temp", [1.0, 0.5])
@pytest.mark.parametrize("win", [None, "patch"])
def test_deferred_restatement_equals_forward_on_the_staircase(win, temp):
    """The float32 oracle forward against the float32 deferred restatement on overlap lists: colour, depth and alpha within the
    project's bar, 1e-5 of each tensor's maximum (the two round (c a) T against c (a T)); the figures are printed and recorded
    in DESIGN.md.  Control: on the standard lists (inside all true) alpha differs at silhouette pixels."""
    s = oref.scene("staircase")
    w = oref.full_window(s) if win is None else oref.STAIR_PATCH
    x = oref.evaluate(s, w)
    sel = oref.select(x, oref.STAIR_L)
    fwd = oref.forward32(s, w, temp)
    dfr = oref.deferred32(s, sel, temp, w)
    for k in ("color", "depth_raw", "alpha"):
        d = rel_linf(dfr[k], fwd[k])
        print(f"staircase win={win} temp={temp} {k}: deferred vs forward {d:.3g} of max {np.abs(fwd[k]).max():.3g}")
        assert d <= GRAD_TOL, (k, d)
    pm, pw, ph = w
    std = rref.select(wref.intersect(s, pm, pw, ph), oref.STAIR_L)
    std["inside"] = std["layers"] >= 0
    ctl = oref.deferred32(s, std, temp, w)
    sil = (sel["layers"] >= 0) & ~sel["inside"]
    diff = np.abs(ctl["alpha"].astype(np.float64) - fwd["alpha"]) > GRAD_TOL * np.abs(fwd["alpha"]).max()
    print(f"control: {int(diff.sum())} pixels differ in alpha, {int(sil.any(-1).sum())} silhouette pixels")
    assert diff.any() and not (diff & ~sil.any(-1)).any()
    assert rel_linf(ctl["alpha"], fwd["alpha"]) > 1e-3
