"""The sparse upstream gradients of tests/upstream.py on the CPU: on every scene and family the fp32 oracle stays inside the
acceptance the GPU tests hold the kernels to (tests/test_gpu_sparse_upstream.py), the per-pixel terms add up to the oracle's
gradient, and each family reaches what it is for."""
import numpy as np
import pytest

import upstream as U
from util import GRAD_NAMES, summation_bound

MODES = ("aa", "point", "alpha")


@pytest.mark.parametrize("family", U.IMAGE_FAMILIES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", U.SCENES)
def test_fp32_oracle_inside_the_bound(scene, mode, family):
    """|g32 - g64| <= GRAD_TOL max|g64| + 8 eps32 sum|per-pixel terms| on every element -- the reference alone stays inside the
    criterion on the chosen inputs -- except, on the tie lattice, the elements that receive a term on which the two oracles
    disagree (Context.disagree; counted below); and the terms are the gradient's.  The exact-zero part of the criterion says
    nothing about the fp32 oracle itself: here the elements it makes non-zero where every float64 term is exactly 0 (a clamped
    barycentric weight that rounds) are counted, and they stay within the bound's tolerance term, GRAD_TOL max|g64|."""
    ctx = U.context(scene, mode == "point", family)
    ref = ctx.reference(family, alpha=mode == "alpha")
    total = ctx.terms.sum(ref["mask"], ref["groups"])
    lines = []
    for n in GRAD_NAMES:
        held = None if ref["held32"] is None else ref["held32"][n]
        lines.append(U.check_tensor(n, ref["g32"][n], ref["g64"][n], ref["sabs"][n], g32=ref["g32"][n], held32=held,
                                    what=f"{scene} {mode} {family} fp32 oracle")[0])
        assert (np.abs(total[n] - ref["g64"][n]) <= summation_bound(0.0, ref["sabs"][n])).all(), n   # (the terms sum to the gradient)
        rounded = (ref["sabs"][n] == 0) & (ref["g32"][n] != 0)
        if held is not None:
            rounded &= ~held
            assert held.sum() < held.size, n
        if rounded.any():
            size = float(np.abs(ref["g32"][n][rounded]).max())
            lines.append(f"    {int(rounded.sum())} of {rounded.size} elements non-zero in the fp32 oracle with all float64 terms zero, largest {size:.3g}")
            assert size <= summation_bound(float(np.abs(ref["g64"][n]).max()), 0.0) and 2 * rounded.sum() < rounded.size, n
    print("\n".join(lines))
    if family == "all_zero":
        for x in (ref["gc"], ref["gd"]) + ((ref["gA"],) if ref["gA"] is not None else ()):
            assert not x.any() and np.signbit(x).any() and not np.signbit(x).all()
    else:
        kept = ref["mask"]
        assert not ref["gd"][~kept].any() and not ref["gc"][~kept].any()
        assert kept.any() or family in ("lane63", "lane255")                       # (a lane outside a ragged tile has no pixel)


# ---- what the families are for: the tie lattice ---------------------------------------------------------------------------------
CAND, LANES_PER_CHUNK, WAVE = 30, 256, 64          # k_render_backward_fast<POOL>: candidate entries and pair lanes of a chunk


def _blend_sets(args):
    """Per pixel q of the lattice's one tile: the faces the forward's masks hold for it -- the pairs that blend whatever the
    running T says (the forward sets a mask bit without knowing whether the pixel has terminated in front of the entry).  From
    the fp32 oracle on 1 x 1 patches with every opacity at 1e-3, where no pixel terminates: the faces with a non-zero opacity
    gradient under a dense upstream gradient."""
    from oracle import cpu as orc
    from util import to_numpy_args
    a = to_numpy_args(args)
    W, H = int(a[2]), int(a[3])
    assert a[8].shape[0] == 1 and W <= 16 and H <= 16
    a[7] = np.full_like(a[7], 1e-3)
    rng = np.random.default_rng(5)
    sets = []
    for q in range(256):
        x, y = q & 15, q >> 4
        if x >= W or y >= H:
            sets.append(set()); continue
        b = list(a)
        b[1] = a[1] + np.array([[x, y]], a[1].dtype); b[2] = 1; b[3] = 1
        b[19] = np.ascontiguousarray(a[19][:, y:y + 1, x:x + 1]); b[20] = np.ascontiguousarray(a[20][:, y:y + 1, x:x + 1])
        r = orc.render_forward_cuda(*b)
        g = orc.render_backward_cuda(r, rng.standard_normal((1, 1, 1, 3)).astype(np.float32), rng.standard_normal((1, 1, 1)).astype(np.float32))
        sets.append(set(np.flatnonzero(g["faces_opacity"]).tolist()))
    return sets


_LAYOUT = {}


def _lattice_pairs():
    """The chunks of the lattice tile's backward walk as the kernel cuts them -- the walk runs from the tile's deepest live entry
    to the front, a chunk takes the leading entries of the next CAND whose pairs fit 256 lanes, pair lanes are numbered face by
    face and within a face by pixel -- with, per pair lane: pixel, whether it is active (in front of the pixel's last
    contributor) and whether it is an exact tie (structured.exact_ties on the face's table).
    -> list of chunks, each a list of (lane s, pixel q, active, tie)."""
    if "pairs" not in _LAYOUT:
        import structured as S
        ctx = U.context("lattice")
        sets = _blend_sets(ctx.args)
        bn = ctx.r32.binning
        r0, r1 = int(bn.ranges[0][0]), int(bn.ranges[0][1])
        entries = bn.face_list[r0:r1].astype(np.int64)
        nc = np.zeros((16, 16), np.int64)
        nc[:ctx.H, :ctx.W] = ctx.r32.n_contrib.reshape(ctx.H, ctx.W)
        nc = nc.reshape(-1)
        total = int(min(nc.max(), len(entries)))
        hits = [[q for q in range(256) if int(f) in sets[q]] for f in entries[:total]]
        tv = ctx.na[12][0]
        pm = np.asarray(ctx.na[1], np.float32)[0]
        chunks, base = [], 0
        while base < total:
            cand = [total - 1 - (base + j) for j in range(min(CAND, total - base))]          # list positions, back to front
            cum = np.cumsum([len(hits[e]) for e in cand])
            n = max(1, int((cum <= LANES_PER_CHUNK).sum()))
            pairs, s = [], 0
            for e in cand[:n]:
                f = int(entries[e])
                qs = np.array(hits[e], np.int64)
                if len(qs):
                    pix = np.stack([qs & 15, qs >> 4], 1).astype(np.float32) + pm
                    ties = S.exact_ties(np.broadcast_to(tv[f], (len(qs), 3, 2)), pix)
                    for q, t in zip(qs.tolist(), ties.tolist()):
                        pairs.append((s, q, e < nc[q], bool(t))); s += 1
            assert s <= LANES_PER_CHUNK
            chunks.append(pairs)
            base += n
        _LAYOUT["pairs"] = chunks
    return _LAYOUT["pairs"]


def _pushes(family):
    """Per chunk: the pair lanes whose tie is queued under the family (tie, active, a non-zero upstream gradient at its pixel),
    and the number of active ties whose dL/d(area) is zero."""
    ctx = U.context("lattice")
    ref = ctx.reference(family)
    live = np.zeros((16, 16), dtype=bool)
    live[:ctx.H, :ctx.W] = (ref["mask"] & ((ref["gc"] != 0).any(-1) | (ref["gd"] != 0)))[0]
    live = live.reshape(-1)
    out, zero = [], 0
    for pairs in _lattice_pairs():
        out.append([s for s, q, active, tie in pairs if tie and active and live[q]])
        zero += sum(1 for s, q, active, tie in pairs if tie and active and not live[q])
    return out, zero


@pytest.mark.parametrize("family", ["one_pixel_per_tile", "lane0", "checker"])
def test_lattice_ties_with_and_without_gradient(family):
    """Ties whose upstream dL/d(area) is zero are never queued: both kinds must be there, so the wave's ballot is a proper subset
    of its ties."""
    pushes, zero = _pushes(family)
    queued = sum(len(p) for p in pushes)
    print(f"lattice {family}: {queued} ties queued, {zero} ties with a zero dL/d(area), {len(pushes)} chunks")
    assert queued > 0 and zero > 0, (queued, zero)


def test_lattice_lane0_is_some_waves_only_tie():
    """Under lane0 some wave's ballot is lane 0 alone (tie_first == 0 with nothing behind it).  That is the ballot, not the
    spare-lane choice `tie_first == 0 ? 1 : 0`, which only acts in wave 0 of the tile's LAST chunk while the buffer holds
    entries: no window of the lattice within 8 pixels of its corner puts a tie of pixel 0 into the first lane of the last
    chunk, so under lane0 the last chunk is met with held entries and no tie of its own (tie_first == -1), asserted here too."""
    pushes, _ = _pushes("lane0")
    waves = [sorted(s % WAVE for s in p if s // WAVE == w) for p in pushes for w in range(4)]
    assert [0] in waves, [w for w in waves if w]
    assert not pushes[-1] and 0 < sum(len(p) for p in pushes[:-1]) < 32, [len(p) for p in pushes]   # (held, never drained)


def test_lattice_one_row_leaves_a_chunk_without_ties():
    """Under one_row some chunk queues nothing while an earlier chunk of the walk did (the buffer holds ties from before)."""
    pushes, _ = _pushes("one_row")
    counts = [len(p) for p in pushes]
    print("lattice one_row: ties queued per chunk", counts)
    first = next((i for i, c in enumerate(counts) if c), None)
    assert first is not None and 0 in counts[first + 1:], counts


# ---- the replay stack -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [f for f in U.IMAGE_FAMILIES if f != "all_zero"])
def test_replay_support_holds_a_pixel_whose_records_span_chunks(family):
    """Every family keeps a pixel with more contributors than a chunk has candidate entries: its records come in two chunks at
    least.  (The windows of upstream.window_of put the fixed pixels of the lane families and of one_pixel_per_tile there.)"""
    ctx = U.context("replay", False, family)
    ref = ctx.reference(family)
    deep = ctx.weight > CAND
    assert (deep & ref["mask"]).any(), (family, ctx.window, int(deep.sum()))


# ---- what the material axes are for (upstream.material_args; tests/test_gpu_sparse_upstream.py test_material_axes) --------------
#                 (scene, temp): pixels ending on an alpha-1 contributor, (pixel, face) blends of intensity 0 -- as counted here
MATERIAL_REACH = {("ragged", None): (692, 29), ("ragged", 0.0): (996, 29), ("two_views", None): (962, 35)}


@pytest.mark.parametrize("scene,temp", U.MATERIAL_SCENES, ids=[f"{s}-{'own' if t is None else t}" for s, t in U.MATERIAL_SCENES])
def test_material_axes_reach_what_they_are_for(scene, temp):
    """From the fp32 oracle alone: the pixels whose last contributor has alpha exactly 1 (final_T == 0: the backward's
    alpha_is_one arm, -prev_T_final times the background terms), the faces of intensity exactly 0 whose intensity gradient is
    not zero (they blend: the factor the colour gradients carry and the intensity gradient does not), opacity gradients of
    opacity-0 faces (alpha 0 pairs do not blend and yet have a gradient), a background no channel swap leaves alone; a floor of
    a third of each count.  And the fp32 oracle stays within GRAD_TOL of the float64 one, the GPU test's acceptance."""
    from oracle import cpu as orc
    from util import GRAD_TOL, rel_linf, to_numpy_args
    na = to_numpy_args(U.material_args(scene, temp))
    r32 = orc.render_forward_cuda(*na, nthreads=4)
    r64 = orc.render_forward_cuda(*na, dtype=np.float64, nthreads=4)
    B, H, W = r32.depth.shape
    gc, gd, _ = U.dense_upstream(scene, B, H, W)
    g32 = orc.render_backward_cuda(r32, gc, gd, nthreads=4)
    g64 = orc.render_backward_cuda(r64, gc.astype(np.float64), gd.astype(np.float64), nthreads=4)
    for n in GRAD_NAMES:
        assert rel_linf(g32[n], g64[n]) <= GRAD_TOL / 2, n
    nc, fT = r32.n_contrib.reshape(-1), r32.final_T.reshape(-1)
    opaque_last = int(((nc > 0) & (fT == 0.0)).sum())
    dark = int(((na[10] == 0.0) & (g32["faces_intense"] != 0.0)).sum())
    clear = int(((na[7] == 0.0) & (g32["faces_opacity"] != 0.0)).sum())
    opaque = int(((na[7] == 1.0) & (g32["faces_opacity"] != 0.0)).sum())
    print(f"materials {scene} {temp}: {opaque_last} of {nc.size} pixels end on an alpha-1 contributor, {dark} (view, face) of "
          f"intensity 0 blend, {clear} faces of opacity 0 and {opaque} of opacity 1 have an opacity gradient")
    want = MATERIAL_REACH[(scene, temp)]
    assert opaque_last >= want[0] // 3, opaque_last
    assert dark >= max(want[1] // 3, 1) and clear >= 1 and opaque >= 1, (dark, clear, opaque)
    bg = na[0]
    assert bg.min() < 0 and bg.max() > 1 and len(set(bg.tolist())) == 3 and (np.abs(na[6]).max() <= 1) and (na[6] < 0).any()


VANISHING_REACH = 520          # pixels of the ragged scene that end on another face than under a usable temperature, as counted here


def test_vanishing_temperature_reaches_pairs_of_zero_coverage():
    """From the fp32 oracle alone: under aa_temperature = 2^-149 the pixels whose last contributor differs from the one under
    2^-100 (where no product rounds to 0) -- pixels that own a pair whose mixed coverage is exactly 0 behind their last
    blending one; a floor of a third of the count.  The records are the same (a pair of zero mixed coverage still has an area)."""
    from oracle import cpu as orc
    from util import to_numpy_args
    a = to_numpy_args(U.scene_args("ragged", U.VANISHING_TEMPERATURE))
    b = to_numpy_args(U.scene_args("ragged", float(np.float32(2.0 ** -100))))
    assert 0.0 < a[11] < 1e-44 and np.float32(a[11]) * np.float32(0.5) == 0 and np.float32(a[11]) * np.float32(0.75) != 0
    ra, rb = orc.render_forward_cuda(*a), orc.render_forward_cuda(*b)
    moved = int((ra.n_contrib != rb.n_contrib).sum())
    print(f"vanishing temperature: {moved} of {ra.n_contrib.size} pixels end on another face")
    assert moved >= VANISHING_REACH // 3 and (ra.n_contrib <= rb.n_contrib).all()
    assert np.array_equal(ra.buf_tri_cnt, rb.buf_tri_cnt)
