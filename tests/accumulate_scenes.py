"""Hand-built scenes for how the backward's phase D delivers a face's partial sums (tests/test_gpu_backward_accumulate.py,
tests/test_backward_accumulate_scenes.py): one emit per face and wave, whatever 16-lane rows the face's pair lanes cross.

One 16 x 16 tile, image space = world space as in tests/backward_replay_scenes.py (its make_args: face i lies in front of face
i + 1, rays along +z through the pixel centres).  A chunk's pair lanes are face-major in walk order -- deepest entry first, a
face's pairs next to each other -- so a face with n pairs is a run of n lanes, and where it starts is the sum of the pairs of
the faces behind it.  ``layout`` replays that cut from the oracle's forward state alone (tile list, n_contrib, the per-pixel
lists of faces with a live overlap): the chunks of the tile and, per chunk, the face of every one of its 256 pair lanes.
Nothing of the library is involved, and the ``present_*`` functions assert from it that the situation a scene exists for
is there."""
import functools

import numpy as np

import backward_replay_scenes as R

W = H = 16
CAND = 30                      # candidate entries per chunk of the default backward (DM2_BF_CAND; 32 without a pair pool)
CHUNK_LANES = 256


def _row_sliver(row, x0, n):
    """A face inside pixel row ``row`` that overlaps exactly the n pixels x0 .. x0 + n - 1."""
    return [(x0 + 0.3, row + 0.4), (x0 + n - 0.3, row + 0.42), (x0 + 0.5 * n, row + 0.63)]


def _band(row, x_apex, y_apex, x_left=-4.0, y_low=1.8):
    """A face over rows ``row`` and ``row + 1`` from the tile's left edge to its apex: both rows up to the apex' pixel where the
    apex is at row + 1, fewer pixels of the lower row where it is above; ``y_low`` > 2 dips into row + 2 at the left edge."""
    return [(x_left, row + 0.2), (x_apex, row + y_apex), (x_left, row + y_low)]


# n pairs -> a face with that many, at pixel row ``row`` (the counts are asserted from the oracle, not trusted)
def face_of(n, row):
    if n <= 16:
        return _row_sliver(row, 0, n)
    if n == 17:                                      # a full row and the pixel the apex dips into
        return [(0.3, row + 0.4), (15.7, row + 0.42), (7.5, row + 1.02)]
    if n == 31:                                      # 16 + 15: the lower edge leaves row + 1 inside pixel 14
        return _band(row, 15.5, 0.95)
    if n == 32:
        return _band(row, 20.0, 1.0)
    if n == 33:                                      # 32 and pixel 0 of row + 2
        return _band(row, 20.0, 1.0, x_left=-0.5, y_low=2.05)
    raise ValueError(n)


# walk order (deepest first): the run of 17 has the row boundary 15|16 inside and ends at a row's last lane (31); 16 fills a row
# exactly; 33 crosses the wave boundary 63|64 and ends on lane 80, a row's first; 32 crosses 127|128; the second 16 ends at
# wave 2's last lane (191); the last face ends at lane 255
BOUNDARY_RUNS = [15, 17, 16, 33, 31, 32, 17, 15, 16, 33, 31]
BOUNDARY_ROWS = [0, 1, 3, 4, 7, 9, 11, 13, 14, 0, 5]            # where each sits in the tile (faces may share pixels)


def _make(tris_walk_order, temp, seed, opac_lo=0.15, opac_hi=0.45):
    """faces given deepest first -> make_args wants them nearest first"""
    tris = [np.asarray(R._snap(t)) for t in reversed(tris_walk_order)]
    rng = np.random.default_rng(seed)
    return R.make_args(tris, rng.uniform(opac_lo, opac_hi, len(tris)), W, H, temp, seed=seed + 1)


def covering(temp=1.0):
    """Scene 1: one face over the whole tile, 256 pairs: its run spans all four rows of every wave and all four waves."""
    return _make([[(-20.0, -20.0), (60.0, -20.0), (-20.0, 60.0)]], temp, 501)


def boundaries(temp=1.0):
    """Scene 2: faces of exactly 15, 16, 17, 31, 32 and 33 pairs, 256 in all (BOUNDARY_RUNS)."""
    return _make([face_of(n, r) for n, r in zip(BOUNDARY_RUNS, BOUNDARY_ROWS)], temp, 502)


STACK = 32


def covering_stack(temp=1.0):
    """A 64 x 32 frame, eight tiles, under 32 faces that each cover all of it: eight list entries a face, 256 pairs an entry."""
    rng = np.random.default_rng(504)
    tris = [R._snap(np.array([(-40.0, -40.0), (200.0, -40.0), (-40.0, 200.0)]) + rng.uniform(-2, 2, (3, 2))) for _ in range(STACK)]
    return R.make_args(tris, rng.uniform(0.03, 0.08, STACK), 64, 32, temp, seed=505)


ROW_ROUTE_TILES_PER_FACE = 3   # dm2_backward_fast.hip: list entries per (view, face) from which the default backward takes the row route


def route(args, ref):
    """Which instantiation of the default backward the launcher picks for this frame: list entries (as it reads them off the
    binning scratch: rounded up to 64, less 63) against ROW_ROUTE_TILES_PER_FACE per (view, face)."""
    entries = -(-int(ref.num_rendered) // 64) * 64 - 63
    views, faces = ref.depth.shape[0], int(args[5].shape[0])
    return "row" if entries >= ROW_ROUTE_TILES_PER_FACE * views * faces else "wide"


STRIP_FACES = 30


def strip(temp=1.0, nan_vertex=False):
    """Scenes 3 and 4: 30 faces of two pixels each, all in the 4-row strip y < 4: 60 pair lanes in one wave, every chunk
    candidate emits from it.  ``nan_vertex``: one world-space corner of the face in the middle of the walk is NaN."""
    tris = []
    for i in range(STRIP_FACES):
        row, x0 = i // 8, 2 * (i % 8)
        tris.append(_row_sliver(row, x0, 2))
    args = _make(tris, temp, 503)
    if nan_vertex:
        v = args[4].clone()
        v[3 * NAN_FACE + 1, 0] = float("nan")
        args[4] = v
    return args


NAN_FACE = 14                  # (index in make_args order: nearest first)


@functools.lru_cache(maxsize=None)
def _cached(name, temp):
    return tuple({"covering": covering, "boundaries": boundaries, "strip": strip, "covering_stack": covering_stack,
                  "strip_nan": functools.partial(strip, nan_vertex=True)}[name](temp))


def make_args(name, temp=1.0):
    return list(_cached(name, float(temp)))


# ---- the backward's chunk cut and pair-lane map, from the oracle's forward state -------------------------------------------------
def pair_pixels(args, ref):
    """-> {face id: sorted pixel indices (y * 16 + x) the forward blends the face into}; aa_temperature > 0: the faces with a
    live overlap (every ray of these scenes meets every face's plane, and the mixed coverage of a positive area is positive)."""
    assert float(args[11]) > 0
    cnt = ref.buf_tri_cnt.reshape(H * W)
    ids = ref.buf_tri_id.reshape(H * W, -1)
    assert (cnt < ids.shape[1]).all()                            # (the per-pixel lists did not overflow)
    out = {}
    for p in range(H * W):
        for f in ids[p, :cnt[p]]:
            out.setdefault(int(f), []).append(p)
    return out


def layout(args, ref, cand=CAND):
    """-> [chunk], chunk = int array (256): the list entry's face id on every pair lane, -1 on the idle ones.  The walk starts at
    the tile's deepest live entry; a chunk keeps the leading candidates (<= cand) whose pairs fit 256 lanes, one at least."""
    r0, r1 = (int(x) for x in ref.binning.ranges[0])
    total = min(int(ref.n_contrib.max()), r1 - r0)
    entries = [int(f) for f in ref.binning.face_list[r0:r0 + total]][::-1]          # walk order
    px = pair_pixels(args, ref)
    chunks, base = [], 0
    while base < total:
        lanes, n = [], 0
        for f in entries[base:base + cand]:
            c = len(px.get(f, ()))
            if len(lanes) + c > CHUNK_LANES:
                break
            lanes += [f] * c
            n += 1
        n = max(n, 1)
        lanes = (lanes + [-1] * CHUNK_LANES)[:CHUNK_LANES]
        chunks.append(np.array(lanes))
        base += n
    return chunks


def run_bounds(keys):
    """[(face, first lane, last lane)] of a chunk's lanes"""
    out, s = [], 0
    for l in range(1, len(keys) + 1):
        if l == len(keys) or keys[l] != keys[l - 1]:
            if keys[s] >= 0:
                out.append((int(keys[s]), s, l - 1))
            s = l
    return out


def emits_per_wave(keys):
    """-> (one emit per face and wave, one per face and 16-lane row) for each of the chunk's four waves"""
    per_wave = [len({k for k in keys[w:w + 64] if k >= 0}) for w in range(0, CHUNK_LANES, 64)]
    per_row = [sum(len({k for k in keys[r:r + 16] if k >= 0}) for r in range(w, w + 64, 16)) for w in range(0, CHUNK_LANES, 64)]
    return per_wave, per_row


def present_covering(args, ref):
    ch = layout(args, ref)
    assert len(ch) == 1 and (ch[0] == ch[0][0]).all() and ch[0][0] >= 0, ch
    return ch


def present_boundaries(args, ref):
    ch = layout(args, ref)
    assert len(ch) == 1
    rb = run_bounds(ch[0])
    assert [e - s + 1 for _, s, e in rb] == BOUNDARY_RUNS, [e - s + 1 for _, s, e in rb]
    inside_row = [(s, e) for _, s, e in rb if s // 16 != e // 16]
    inside_wave = [(s, e) for _, s, e in rb if s // 64 != e // 64]
    assert len(inside_row) >= 6 and len(inside_wave) >= 2                           # a boundary inside the run
    assert any(e % 16 == 15 and s // 16 != e // 16 for s, e in inside_row)          # ... and a row boundary right at its end
    assert any(s % 16 == 0 and e % 16 == 15 and e - s == 15 for _, s, e in rb)      # a run that is exactly one row
    assert any(e % 64 == 63 for _, s, e in rb if e < 255) and rb[-1][2] == 255      # a wave boundary right at a run's end
    assert any(e % 16 == 0 and s // 64 != e // 64 for s, e in inside_wave)          # one lane into the next wave's first row
    return ch


def present_strip(args, ref):
    """Every candidate of the one chunk emits from wave 0: 30 emit lanes in one wave, the most a wave can have (a chunk has 30
    candidates), every one of them a face that owns its accumulator row."""
    ch = layout(args, ref)
    assert len(ch) == 1
    per_wave, per_row = emits_per_wave(ch[0])
    assert per_wave[0] == STRIP_FACES == CAND and per_wave[1:] == [0, 0, 0], per_wave
    assert (ch[0][:2 * STRIP_FACES] >= 0).all() and (ch[0][2 * STRIP_FACES:] < 0).all()
    return ch
