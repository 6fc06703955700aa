"""The scenes of tests/tie_queue_scenes.py run through the oracle: something is rendered, the forward and every gradient are
finite, and the lattice scenes do send gradient to the AA tables (their faces are what the tie path is for)."""
import numpy as np
import pytest

import tie_queue_scenes as TQ
from util import to_numpy_args


@pytest.mark.parametrize("name", sorted(TQ.SCENES))
def test_scene_runs_through_the_oracle(name):
    from oracle import cpu as orc
    args = TQ.make_args(name)
    nt = min(orc.max_threads(), 16)
    ref = orc.render_forward_cuda(*to_numpy_args(args), nthreads=nt)
    assert ref.num_rendered > 0
    assert np.isfinite(ref.color).all() and np.isfinite(ref.depth).all()
    rng = np.random.RandomState(1)
    gc = rng.randn(*ref.color.shape).astype(np.float32); gd = rng.randn(*ref.depth.shape).astype(np.float32)
    grads = orc.render_backward_cuda(ref, gc, gd, nthreads=nt)
    for k, g in grads.items():
        assert np.isfinite(g).all(), k
    assert np.abs(grads["aa_face_verts"]).max() > 0
