"""How phase D of the mask-driven backward (dm2_backward_fast.hip) delivers a face's partial sums: the segmented scan runs
across the wave's 16-lane rows and a face emits once per wave.  Scenes built for it (tests/accumulate_scenes.py; each case first
asserts from the oracle's forward state that its lane layout is there): one face on all 256 pair lanes, faces of 15 .. 33
pairs whose runs have row and wave boundaries inside them and right at their end, a wave in which all 30 chunk candidates emit,
the same with a NaN vertex, and the boundary scene on every other instantiation of the kernel.

Bars, as in test_gpu_structured.py: forward outputs and integer state bit-exact, all six gradients within GRAD_TOL = 1e-5
relative L-inf of the oracle with the same non-finite pattern."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import accumulate_scenes as A
from util import (GRAD_NAMES, GRAD_TOL, check_backward, check_forward, check_from_image, rel_linf, run_both, to_dev,
                  to_numpy_args)

from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _flags(f):
    old = _C.set_flags(f)
    try:
        yield
    finally:
        _C.set_flags(old)


def _nan_pixels_made_equal(res):
    """A NaN vertex reaches the pixels of its face in colour and depth, and a NaN's payload and sign are not the reference's
    to define: where BOTH sides hold a NaN -- the same pixels on either side -- both get 0, so that check_forward compares the
    NaN pattern and every other bit."""
    out, ref = list(res["out"]), copy.copy(res["ref"])
    for i, name in ((1, "color"), (2, "depth")):
        g, r = out[i].cpu().numpy().copy(), getattr(ref, name).copy()
        both = np.isnan(g) & np.isnan(r)
        assert both.sum() == np.isnan(g).sum() == np.isnan(r).sum() > 0, name
        g[both] = 0; r[both] = 0
        out[i] = torch.from_numpy(g).cuda(); setattr(ref, name, r)
    return dict(res, out=tuple(out), ref=ref)


def _both(name, temp=1.0, flags=0, mode=None, nan_pixels=False):
    args = A.make_args(name, temp)
    with _flags(flags):
        res = run_both(args, seed=31)
        assert _C.last_forward_mode() == (_C.FWD_POOL if mode is None else mode)
    check_forward(_nan_pixels_made_equal(res) if nan_pixels else res, args)
    worst = check_backward(res)
    print(f"\n{name} t{temp} flags {flags}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return args, res


def test_one_face_over_the_tile():
    """256 pairs of one face: its run spans all four rows of every wave, and every wave emits once."""
    args, res = _both("covering")
    A.present_covering(args, res["ref"])
    assert all(np.abs(res["ref_grads"][n]).max() > 0 for n in ("verts_color", "faces_opacity", "faces_intense"))


def test_runs_with_row_and_wave_boundaries_inside_and_at_their_end():
    """Faces of exactly 15, 16, 17, 31, 32 and 33 pairs, 256 in one chunk."""
    args, res = _both("boundaries")
    A.present_boundaries(args, res["ref"])


def test_every_chunk_candidate_emits_from_one_wave():
    """30 faces of two pixels in one 4-row strip: 30 emits in wave 0."""
    args, res = _both("strip")
    A.present_strip(args, res["ref"])


def test_nan_vertex_stays_in_its_face():
    """The strip with one NaN world-space corner: the wave takes the select form of the scan; every other face's gradient is
    finite and within the bar (check_backward compares where the oracle is finite and wants the same tensors non-finite)."""
    args, res = _both("strip_nan", nan_pixels=True)
    A.present_strip(args, res["ref"])
    own = np.zeros(len(args[4]), bool); own[3 * A.NAN_FACE:3 * A.NAN_FACE + 3] = True
    face = np.arange(A.STRIP_FACES) == A.NAN_FACE
    g = dict(zip(GRAD_NAMES, res["grads"]))
    assert not np.isfinite(g["verts"][own]).all()
    assert np.isfinite(g["verts"][~own]).all() and np.isfinite(g["verts_color"][~own]).all()
    assert np.isfinite(g["faces_opacity"][~face]).all() and np.isfinite(g["aa_face_verts"][:, ~face]).all()
    assert np.isfinite(g["faces_intense"][:, ~face]).all()


def test_many_large_faces_take_the_row_route():
    """32 faces over a frame of eight tiles: eight list entries a face, over the 3 at which the launcher picks the instantiation
    with runs inside the rows and adds."""
    args, res = _both("covering_stack")
    assert A.route(args, res["ref"]) == "row" and res["ref"].num_rendered == 8 * A.STACK


def test_the_small_scenes_take_the_wide_route():
    from oracle import cpu as orc
    for name in ("covering", "boundaries", "strip"):
        args = A.make_args(name)
        ref = orc.render_forward_cuda(*to_numpy_args(args))
        assert A.route(args, ref) == "wide", name              # (a one-tile frame has one list entry a face)


def test_boundaries_without_a_pair_pool():
    """CLIP: the masks-only instantiation (32 candidates a chunk: the same single chunk)."""
    args, res = _both("boundaries", flags=_C.DM2_FLAG_NO_PAIR_POOL, mode=_C.FWD_MASKS)
    assert len(A.layout(args, res["ref"], cand=32)) == 1


def test_boundaries_point_sampled():
    """POINT: temperature 0, no AA components; the two-row faces still give runs longer than a row."""
    import backward_replay_scenes as R
    args, res = _both("boundaries", temp=0.0, mode=_C.FWD_POINT)
    # at temperature 0 a pair is a pixel whose centre the face covers: n_contrib counts them, and the two-row faces keep more
    # than a row's 16 of them (float64 geometry of the very arguments the kernels got)
    centres = [int(R._centre_inside(t, A.W, A.H).sum()) for t in R._tris(args)]
    assert sum(c > 16 for c in centres) >= 2, centres
    nc = res["ref"].n_contrib.reshape(A.H, A.W)
    for t, c in zip(R._tris(args), centres):
        if c > 16:
            assert (nc[R._centre_inside(t, A.W, A.H)] >= 1).all()                  # the oracle blended there


def test_boundaries_with_the_alpha_images_gradient():
    """ALPHA: colour, depth and alpha losses together, against the sum of the oracle's two backwards."""
    from test_gpu_backward_replay import _run_alpha
    from oracle import cpu as orc
    args = A.make_args("boundaries")
    ref = orc.render_forward_cuda(*to_numpy_args(args))
    A.present_boundaries(args, ref)
    kz = np.zeros((A.H, A.W), bool); kz[5, 3] = True
    grads, want = _run_alpha(args, ref, kz)
    worst = {}
    for name, x in zip(GRAD_NAMES, grads):
        assert x.shape == want[name].shape and np.isfinite(x).all(), name
        worst[name] = rel_linf(x, want[name])
    print("\nboundaries alpha:", worst)
    assert all(v <= GRAD_TOL for v in worst.values()), worst


def test_boundaries_aa_gradient_routed_to_the_vertices():
    """aa_grad_to_verts on the default op path (tables from verts_image): the flush sends a face's six AA sums to its vertices."""
    from oracle import cpu as orc
    from util import from_image_oracle_args
    cpu_args = A.make_args("boundaries")
    # the layout on THIS path: the oracle on the tables rebuilt from verts_image, as check_from_image runs it
    oargs = from_image_oracle_args(cpu_args)
    A.present_boundaries(cpu_args, orc.render_forward_cuda(*oargs))
    args = to_dev(cpu_args)
    g = torch.Generator().manual_seed(11)
    wc = torch.randn((1, A.H, A.W, 3), generator=g).cuda(); wd = torch.randn((1, A.H, A.W), generator=g).cuda()
    worst = check_from_image(args, wc, wd, tol=GRAD_TOL)
    print("\nboundaries from-image:", worst)
