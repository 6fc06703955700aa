"""The backward's one-emit-per-face-and-wave rule on the CPU: tests/seg_scan_model.py restates the step words, the six scan
steps and the emit predicate as dm2_dpp.h / dm2_backward_fast.hip form them; here every maximal run of a wave must leave
exactly one emit, on its last lane, that carries the run's whole sum -- whatever rows the run crosses."""
import numpy as np
import pytest

import seg_scan_model as M


def _layout(lengths, idle=0):
    """keys of a wave from run lengths (in lane order): run i has key i; ``idle`` trailing lanes have key -1."""
    keys = []
    for i, n in enumerate(lengths):
        keys += [i] * n
    keys += [-1] * idle
    assert len(keys) == 64, (lengths, idle)
    return np.array(keys)


def _random_layouts(rng, count):
    """Run layouts of 64 lanes with up to 30 keys, as a chunk's face-major pair lanes give them: ascending keys, then idle lanes."""
    for _ in range(count):
        nk = int(rng.randint(1, 31))
        used = int(rng.randint(nk, 65))
        cuts = np.sort(rng.choice(np.arange(1, used), nk - 1, replace=False)) if nk > 1 else np.array([], int)
        lengths = np.diff(np.concatenate([[0], cuts, [used]])).tolist()
        yield _layout(lengths, 64 - used)


def _wave_slices(lengths):
    """The 64-lane windows of a chunk whose faces have ``lengths`` pairs (pair lanes are face-major): keys per wave."""
    keys = np.concatenate([np.full(n, i) for i, n in enumerate(lengths)])
    keys = np.concatenate([keys, np.full(-len(keys) % 64, -1)])
    return [keys[w:w + 64] for w in range(0, len(keys), 64)]


# the layouts of the GPU scenes (tests/accumulate_scenes.py): one face on all 256 lanes; faces of 15, 16, 17, 31, 32, 33 pairs
# whose runs have a row or a wave boundary inside them and right at their end
SCENE_LAYOUTS = _wave_slices([256]) + _wave_slices([15, 17, 16, 33, 31, 32, 17, 15, 16, 33, 31]) \
    + [_layout([2] * 30, 4), _layout([1] + [2] * 29, 5)]


def _check(keys, rng, form):
    vals = rng.randint(-8, 9, 64).astype(np.float64)                          # (small integers: every order sums exactly)
    active = rng.rand(64) < 0.7
    active[keys < 0] = False
    vals[~active] = 0.0                                                       # as the kernel: an inactive lane adds zeros
    cont = M.cont_word(keys)
    got = M.seg_scan64(vals, cont, form)
    emit = M.emits(keys, active, cont)
    for s, e in M.runs(keys):
        want = keys[s] >= 0 and active[s:e + 1].any()
        assert emit[s:e + 1].sum() == (1 if want else 0), (keys.tolist(), s, e)
        if want:
            assert emit[e] and got[e] == vals[s:e + 1].sum(), (keys.tolist(), s, e)
        # every lane holds the inclusive sum of its run (what the row steps plus the two carries promise)
        assert np.array_equal(got[s:e + 1], np.cumsum(vals[s:e + 1])), (keys.tolist(), s, e)


@pytest.mark.parametrize("form", ["fast", "select"])
def test_one_emit_per_run_carries_the_runs_sum(form):
    rng = np.random.RandomState(20261020)
    for keys in list(_random_layouts(rng, 1500)) + SCENE_LAYOUTS:
        _check(np.asarray(keys), rng, form)


def test_runs_by_contiguity_not_by_key():
    """A key that comes back after another one starts a new run (the predicate is "continues the lane before")."""
    rng = np.random.RandomState(7)
    for _ in range(300):
        keys = np.repeat(rng.randint(0, 3, 64), rng.randint(1, 20, 64))[:64]
        _check(keys, rng, "fast")
        _check(keys, rng, "select")


def test_select_form_keeps_a_non_finite_value_in_its_run():
    rng = np.random.RandomState(3)
    for keys in SCENE_LAYOUTS + list(_random_layouts(rng, 200)):
        keys = np.asarray(keys)
        vals = rng.randint(-8, 9, 64).astype(np.float64)
        rr = M.runs(keys)
        s, e = rr[int(rng.randint(len(rr)))]
        bad = int(rng.randint(s, e + 1))
        vals[bad] = np.inf if rng.rand() < 0.5 else np.nan
        got = M.seg_scan64(vals, M.cont_word(keys), "select")
        for a, b in rr:
            if (a, b) == (s, e):
                assert not np.isfinite(got[bad:b + 1]).any() and np.isfinite(got[a:bad]).all()
            else:
                assert np.array_equal(got[a:b + 1], np.cumsum(vals[a:b + 1])), (keys.tolist(), a, b)


def test_runs_cut_at_the_rows_emit_once_per_face_and_row():
    """With the bits of lanes 16, 32, 48 cleared in the ballot (dm2_dpp.h says a caller may) the same steps sum inside the rows,
    no cross-row step is taken, and every (face, row) emits its own part."""
    rng = np.random.RandomState(9)
    for keys in list(_random_layouts(rng, 300)) + SCENE_LAYOUTS:
        keys = np.asarray(keys)
        cont = M.cont_word(keys) & ~M.ROW_FIRST
        k = M.seg_steps(cont)
        assert k["b15"] == 0 and k["b31"] == 0
        vals = rng.randint(-8, 9, 64).astype(np.float64)
        active = keys >= 0
        vals[~active] = 0.0
        got, emit = M.seg_scan64(vals, cont), M.emits(keys, active, cont)
        for s, e in M.runs(keys):
            for r0 in range(s & ~15, e + 1, 16):
                a, b = max(s, r0), min(e, r0 + 15)
                assert emit[a:b + 1].sum() == (1 if keys[s] >= 0 else 0) and (keys[s] < 0 or emit[b])
                assert got[b] == vals[a:b + 1].sum()


def test_a_face_that_stores_has_one_emitting_wave():
    """Phase D stores (no add) for every face but the two the scan names per wave: such a face has lanes in no other wave, so
    its one emit is the only writer of its accumulator row; a named face has lanes in a neighbouring wave."""
    rng = np.random.RandomState(5)
    layouts = [[256], [15, 17, 16, 33, 31, 32, 17, 15, 16, 33, 31], [2] * 30, [64, 64, 64, 64], [63, 2, 63, 2, 126]]
    for _ in range(400):
        pairs = []
        while len(pairs) < 30:
            c = int(rng.choice([0, 1, 2, 5, 9, 16, 40, 64, 65, 130, 256]))
            if sum(pairs) + c > 256:
                break
            pairs.append(c)
        layouts.append(pairs)
    for pairs in layouts:
        end = np.cumsum(pairs); first = end - np.asarray(pairs)
        for w in range(4):
            named = set(M.crossing_faces(pairs, w)) - {-1}
            for j, c in enumerate(pairs):
                here = c > 0 and first[j] < 64 * w + 64 and end[j] > 64 * w
                if not here:
                    assert j not in named, (pairs, w, j)
                    continue
                elsewhere = first[j] < 64 * w or end[j] > 64 * w + 64
                assert (j in named) == elsewhere, (pairs, w, j)


def test_step_words_against_their_definition():
    """b_K: lane l - K is in l's row and run; b15 / b31: the run reaches back to the row's (half's) first lane and beyond."""
    rng = np.random.RandomState(11)
    for keys in list(_random_layouts(rng, 300)) + SCENE_LAYOUTS:
        keys = np.asarray(keys)
        k = M.seg_steps(M.cont_word(keys))
        start = np.zeros(64, int)
        for s, e in M.runs(keys):
            start[s:e + 1] = s
        for l in range(64):
            for K in (1, 2, 4, 8):
                assert bool(k[f"b{K}"] >> l & 1) == ((l & 15) >= K and start[l] <= l - K)
            assert bool(k["b15"] >> l & 1) == (bool(l & 16) and start[l] < (l & ~15))
            assert bool(k["b31"] >> l & 1) == (l >= 32 and start[l] < 32)
