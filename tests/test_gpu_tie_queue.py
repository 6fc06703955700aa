"""The default backward's tie path by the route a tie takes (tests/tie_queue_scenes.py): phase D of k_render_backward_fast<POOL>
puts a tile's ties into a 64-entry LDS buffer, the flush phase moves the buffer to the global queue once it holds 32 entries,
what no longer fits the buffer goes to the queue directly (the overflow route), and in the tile's last chunk the waves and what
the buffer still holds take their places in the queue during phase D; k_aa_ties then adds one face per lane group, to the face
rows or -- under aa_grad_to_verts -- the rows of the face's vertices.

Bars as in test_gpu_structured.py: forward outputs and integer state bit-exact, all six gradients within GRAD_TOL = 1e-5 relative
L-inf of the oracle, the routed AA gradient within 1e-5 of the fp64 scatter.  Each case also asserts the two witness words the
last block of k_aa_ties leaves behind (debug_fetch item 10): [4] the queue length it saw, [5] how many of those entries took
the overflow route.

The scenes are not the lattice grids with every vertex on a pixel corner one would reach for first: the reference's clipper
gives most of their partly covered pairs an error code (never blended), and the pixels left are covered whole (no gradient):
measured on the oracle, tests/tie_queue_scenes.py says what is used instead and why."""
import functools

import numpy as np
import pytest
import torch

import tie_queue_scenes as TQ
from util import (GRAD_TOL, check_backward, check_forward, check_from_image, check_pool, pool_state, rel_linf,
                  run_both, run_from_image, to_dev, to_numpy_args)

pytestmark = pytest.mark.gpu


def _C():
    from dmesh2_renderer_amd import _C as c
    return c


def _nthreads():
    from oracle import cpu as orc
    return min(orc.max_threads(), 16)


def witness(out):
    """hit_valid[0..7] of the forward ``out`` as its last backward's tie pass left them."""
    C = _C()
    B, H, W = out[2].shape
    hv = C.debug_fetch(10, B * H * W, C._tiles(B, W, H), out[0], out[8], torch.int32, 8).cpu().numpy().view(np.uint32)
    assert hv[2] == 0 and hv[3] == 0 and hv[6] == 0, hv                       # the last block emptied the queue and its counters
    return int(hv[4]), int(hv[5])


@functools.lru_cache(maxsize=None)
def _parity(name):
    """Forward bit-exact, six gradients within GRAD_TOL (materialised tables) -> the witness words."""
    args = TQ.make_args(name)
    res = run_both(args, seed=7, nthreads=_nthreads())
    check_forward(res, args)
    worst = check_backward(res)
    n, direct = witness(res["out"])
    print(f"\n{name}: queue length {n}, direct {direct}; " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return n, direct


def test_direct_route():
    """Chunks with far more than 64 ties: the buffer fills and the rest takes the overflow route."""
    n, direct = _parity("direct")
    assert direct > 0 and n >= 256, (n, direct)


def test_end_of_tile_drain_only():
    """Fewer than 32 ties in the frame: no threshold drain, no overflow; a tile's ties leave in its last chunk, those of earlier
    chunks from the buffer."""
    n, direct = _parity("tail")
    assert 0 < n < 32 and direct == 0, (n, direct)


def test_threshold_drains_mid_tile():
    """The tile's ties come over several chunks, a few at a time: the buffer is drained at its threshold and never fills."""
    n, direct = _parity("threshold")
    assert n > 64 and direct == 0, (n, direct)


def test_no_ties():
    """No tie in the frame: every block of the tie pass leaves at once, and the gradients match."""
    n, direct = _parity("none")
    assert n == 0 and direct == 0, (n, direct)


def test_views_and_windows():
    """B = 2 with different patch_min, 32x32 windows of a 64x48 frame, through the default op path: both emit shapes of k_aa_ties
    (face rows, then the vertex rows of a mesh with shared vertices)."""
    args = to_dev(TQ.make_args("windows"))
    g = torch.Generator().manual_seed(11)
    B, ph, pw = args[9].shape[0], int(args[3]), int(args[2])
    assert B == 2 and (ph, pw) == (32, 32) and not torch.equal(args[1][0], args[1][1])
    wc = torch.randn((B, ph, pw, 3), generator=g).cuda(); wd = torch.randn((B, ph, pw), generator=g).cuda()
    worst = check_from_image(args, wc, wd, tol=GRAD_TOL, nthreads=_nthreads())
    out = run_from_image(args, wc, wd)[0]                                    # (its last backward: routed to the vertex rows)
    n, direct = witness(out)
    print(f"\nwindows: queue length {n}, direct {direct}; " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert n >= 256 and direct > 0, (n, direct)


def test_two_backwards_of_one_forward():
    """The second backward of a forward finds the queue, the buffer count and the direct-route count as the first did."""
    from oracle import cpu as orc
    C = _C()
    args = TQ.make_args("direct")
    dargs = to_dev(args)
    out = C.render_forward_cuda(*dargs)
    check_pool(pool_state(out))
    ref = orc.render_forward_cuda(*to_numpy_args(args), nthreads=_nthreads())
    rng = np.random.RandomState(5)
    gc = rng.randn(*ref.color.shape).astype(np.float32); gd = rng.randn(*ref.depth.shape).astype(np.float32)
    gref = orc.render_backward_cuda(ref, gc, gd, nthreads=_nthreads())
    bw = (out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(), out[7], out[8], out[9], out[3], out[4], out[5], out[6])
    runs, words = [], []
    for _ in range(2):
        runs.append([x.cpu().numpy() for x in C.render_backward_cuda(*bw)])
        words.append(witness(out))
    for grads in runs:
        check_backward(dict(grads=grads, ref_grads=gref))
    assert words[0] == words[1] and words[0][0] >= 256 and words[0][1] > 0, words
    for a, b in zip(*runs):
        m = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), m) and rel_linf(a[m], b[m]) <= GRAD_TOL
