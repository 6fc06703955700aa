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


THRESHOLD_REACH = {"16x16": 45, "40x24": 43}          # pixels whose T behind TH_B is (1 - a)(1 - b), as counted here


@pytest.mark.parametrize("temp", [1.0, 0.0])
@pytest.mark.parametrize("frame", list(brs.FRAMES))
def test_threshold_scene_lands_on_T_EPS(frame, temp):
    """From the fp32 oracle alone: on the pixels the two threshold faces and the face behind them cover fully, the transmittance
    behind the second is T_EPS to the bit (step 0: the pixel goes on, n_contrib beyond that face), one ulp below (-1: the pixel
    ends there, final_T is that T) or above (+1); a floor of a third of the pixels counted when the scene was built."""
    orc = _orc()
    for step in brs.THRESHOLD_STEPS:
        args, info = brs.threshold_scene(frame, step, temp)
        ref = orc.render_forward_cuda(*to_numpy_args(args))
        full = brs.present_threshold(args, ref, info)
        print(f"threshold {frame} temp {temp} step {step}: {int(full.sum())} pixels, n_contrib {sorted(set(ref.n_contrib.reshape(full.shape)[full].tolist()))}")
        assert full.sum() >= max(THRESHOLD_REACH[frame] // 3, 6), int(full.sum())
        if step == 0:                                  # the other side of the comparison would have ended these pixels at TH_B
            assert (ref.n_contrib.reshape(full.shape)[full] != brs.TH_B + 1).all()
