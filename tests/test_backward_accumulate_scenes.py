"""The scenes of tests/accumulate_scenes.py run through the oracle alone: the lane layout each one exists for is there (runs
that cross row and wave boundaries, runs that end on them, a wave in which every chunk candidate emits), and the oracle's
gradients are finite except where the NaN scene says otherwise."""
import numpy as np
import pytest

import accumulate_scenes as A
import seg_scan_model as M
from util import to_numpy_args


def _ref(name, temp=1.0):
    from oracle import cpu as orc
    args = A.make_args(name, temp)
    return args, orc.render_forward_cuda(*to_numpy_args(args), nthreads=min(orc.max_threads(), 16))


def _grads(ref):
    from oracle import cpu as orc
    rng = np.random.RandomState(1)
    gc = rng.randn(*ref.color.shape).astype(np.float32); gd = rng.randn(*ref.depth.shape).astype(np.float32)
    return orc.render_backward_cuda(ref, gc, gd)


def test_covering_one_run_over_every_row_and_wave():
    args, ref = _ref("covering")
    ch = A.present_covering(args, ref)
    assert A.emits_per_wave(ch[0]) == ([1, 1, 1, 1], [4, 4, 4, 4])
    assert all(np.isfinite(g).all() for g in _grads(ref).values())


def test_boundaries_runs_of_15_to_33_pairs():
    args, ref = _ref("boundaries")
    ch = A.present_boundaries(args, ref)
    per_wave, per_row = A.emits_per_wave(ch[0])
    assert sum(per_wave) < sum(per_row)
    assert all(np.isfinite(g).all() for g in _grads(ref).values())
    # the model of the kernel's predicate on these very lanes: one emit per face and wave
    for w in range(4):
        keys = ch[0][64 * w:64 * w + 64]
        assert int(M.emits(keys, keys >= 0).sum()) == per_wave[w]


@pytest.mark.parametrize("temp", [0.5, 0.0])
def test_boundaries_at_other_temperatures(temp):
    """The pair sets do not depend on a temperature > 0; at 0 a pair is a pixel centre inside the face, and the two-row faces
    still give runs longer than a row."""
    import backward_replay_scenes as R
    args, ref = _ref("boundaries", temp)
    assert ref.num_rendered == len(A.BOUNDARY_RUNS)
    if temp > 0:
        A.present_boundaries(args, ref)
    else:
        tris = R._tris(args)
        assert sum(int(R._centre_inside(t, A.W, A.H).sum()) > 16 for t in tris) >= 2


def test_strip_every_candidate_emits_from_one_wave():
    args, ref = _ref("strip")
    A.present_strip(args, ref)
    assert all(np.isfinite(g).all() for g in _grads(ref).values())


def test_strip_nan_only_the_nan_faces_rows_are_non_finite():
    args, ref = _ref("strip_nan")
    A.present_strip(args, ref)
    g = _grads(ref)
    own = np.zeros(len(args[4]), bool); own[3 * A.NAN_FACE:3 * A.NAN_FACE + 3] = True
    assert not np.isfinite(g["verts"][own]).all()
    assert np.isfinite(g["verts"][~own]).all() and np.isfinite(g["verts_color"][~own]).all()
    face = np.arange(A.STRIP_FACES) == A.NAN_FACE
    assert np.isfinite(g["faces_opacity"][~face]).all() and np.isfinite(g["aa_face_verts"][:, ~face]).all()
