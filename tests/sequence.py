"""The scene sequence of the training-loop tests (tests/test_gpu_training_loop.py): scenes of ONE shape (B, W, H, F, P), so that
every step of the sequence meets the binning buffer the step before it left behind (``_C._bin_hint``, key (device, B, W, H, F)).

    S0, S1   depth complexity 3        two ordinary steps of about the same size (the second fits the first's buffer)
    S2, S3   depth complexity 60       the scene grew (plan, allocate, run), then stays
    S4       depth complexity 0.3      the scene shrank: every offset inside the buffer moves, the hint shrinks
    S5       S1 behind the far plane   nothing is rendered between two ordinary steps
    S6       S0 again
    T0, T1   S0 at aa_temperature 0, then at 1: the binning part fits, only the pair pool is missing

tests/test_sequence_cpu.py holds the sequence to the conditions that make the GPU tests mean something, on the CPU oracle's
binning, so that a change of scenes.py cannot quietly empty them."""
import functools

import torch

from util import capture_forward_args, scenes

W, H, F, CAMS = 160, 128, 1500, 2
VIEWS = [0, 1]
#        name: (depth complexity, seed offset, moved behind the far plane)
STEPS = {"S0": (3.0, 1, False), "S1": (3.0, 2, False), "S2": (60.0, 3, False), "S3": (60.0, 4, False), "S4": (0.3, 5, False),
         "S5": (3.0, 2, True), "S6": (3.0, 1, False)}
ORDER = ["S0", "S1", "S2", "S3", "S4", "S5", "S6"]
FAR_SHIFT = 20.0


def scene(name):
    """The SoupScene of a step (CPU tensors; a fresh object per call)."""
    dc, seed, far = STEPS[name]
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + 900 + seed, num_cams=CAMS, shared_verts=True, depth_complexity=dc)
    if far:
        sc.verts = sc.verts.clone()
        sc.verts[:, 2] -= FAR_SHIFT
    return sc


@functools.lru_cache(maxsize=None)
def _args(name, temp):
    return tuple(capture_forward_args(scene(name), VIEWS, [[0, 0]] * len(VIEWS), W, H, temp)[0])


def step_args(name, temp=1.0):
    """The 21 boundary arguments of a step (CPU tensors, materialised AA tables, both views, full-frame patch)."""
    return [a.clone() if torch.is_tensor(a) else a for a in _args(name, float(temp))]


def binning(name):
    """The CPU oracle's binning of a step -> (num_rendered, longest tile list, P, F)."""
    from oracle import cpu as orc
    a = [x.numpy() if torch.is_tensor(x) else x for x in _args(name, 1.0)]
    B, P, Fa = a[8].shape[0], a[4].shape[0], a[5].shape[0]
    b = orc.Binning(B, P, Fa, int(a[2]), int(a[3]), a[1], a[5], a[8], a[9])
    longest = int((b.ranges[:, 1].astype("int64") - b.ranges[:, 0]).max()) if b.num_rendered else 0
    return b.num_rendered, longest, P, Fa
