"""The reference's record-stack desync corner, constructed: the scene of
tests/test_gpu_coverage.py::test_record_stack_desync_corner_size_of_the_deviation, shared with the comparisons against the
reference's own kernels (tests/reference_scenes.py).  Nothing here calls the GPU."""
from util import capture_forward_args, scenes

W, H, F = 64, 48, 300
EVERY = 7                               # every seventh face has a degenerate world triangle


def desync_args(K):
    """A scene in which every seventh face has a degenerate WORLD triangle (p1 == p0: the ray test's denominator is exactly 0,
    auxiliary.h:232) under unchanged image-space tables: such a face overlaps its pixels (the forward takes an AA record for
    it, forward.cu:344-352) but never blends.  Where it is the last face of a pixel's list, the reference's backward finds
    its record on top of the stack, does not pop it (the entry lies behind the last contributor, backward.cu:219-221) and so
    never reaches the records of the faces that did blend: that pixel's gradients are lost (with K > 0 only)."""
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + 61, depth_complexity=4.0)
    args = list(capture_forward_args(sc, [0], [[0, 0]], W, H, 1.0, K)[0])
    verts = args[4].clone()
    for f in range(0, F, EVERY):
        verts[3 * f + 1] = verts[3 * f]
    args[4] = verts
    return args
