"""The scenes of tests/test_gpu_backward_replay.py on the CPU: each holds the situation it exists for, and the oracle
reproduces itself on it, run to run (one thread against two), within GRAD_TOL."""
import numpy as np
import pytest

import backward_replay_scenes as brs
from util import GRAD_NAMES, GRAD_TOL, rel_linf, to_numpy_args


def _orc():
    from oracle import cpu as orc
    return orc


SCENES = ["stack24", "stack70", "opaque"]


def build(scene, frame, temp):
    if scene == "opaque":
        return brs.opaque_scene(frame, temp)
    return brs.stack_scene(frame, int(scene[5:]), temp)


def present(scene, args, ref, info):
    if scene == "opaque":
        brs.present_guard(args, ref, info)             # (present_opaque is its first step)
    else:
        brs.present_stack(args, ref, info)


@pytest.mark.parametrize("temp", [1.0, 0.0])
@pytest.mark.parametrize("frame", list(brs.FRAMES))
@pytest.mark.parametrize("scene", SCENES)
def test_scene_holds_its_case_and_oracle_repeats(scene, frame, temp):
    orc = _orc()
    args, info = build(scene, frame, temp)
    na = to_numpy_args(args)
    ref = orc.render_forward_cuda(*na)
    present(scene, args, ref, info)
    ref2 = orc.render_forward_cuda(*na, nthreads=2)
    for k in ("color", "depth", "final_T", "final_prev_T", "n_contrib"):
        assert np.array_equal(getattr(ref, k), getattr(ref2, k)), k
    rng = np.random.RandomState(1)
    gc = rng.randn(*ref.color.shape).astype(np.float32)
    gd = rng.randn(*ref.depth.shape).astype(np.float32)
    g1 = orc.render_backward_cuda(ref, gc, gd)
    g2 = orc.render_backward_cuda(ref2, gc, gd, nthreads=2)
    for name in GRAD_NAMES:
        assert np.abs(g1[name]).max() > 0 or name == "aa_face_verts" and temp == 0.0, name
        assert rel_linf(g2[name], g1[name]) <= GRAD_TOL, name
