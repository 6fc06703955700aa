"""Camera-plane geometry through the module: a lattice of faces with the camera inside it (tests/far.py inside_scene), captured
through the package's own host prep -- the fused HIP prep (the default) and the reference-shaped torch prep.

The reference culls a face only when all three NDC z lie outside [-1, 1] (forward.cu:71), so here faces with a vertex whose |w|
the projection clamped to 1e-4, faces with a vertex behind the camera and faces 1e5 .. 1e6 px across are binned, composited and
differentiated; many of them cover the whole frame.  "inside" is a 64 x 48 frame of a 1 752-face lattice; "crowd" the same frame
of a 46 k-face lattice, whose frame-spanning faces push the plan's pair bound (6.7 k faces per pixel) over the pool budget
(_C._pool_budget, 2^24 pairs here): it keeps blend masks only (DM2_FWD_MASKS) and its backward re-clips every pair.

Bars, as in test_gpu_parity.py: forward bit-exact, the pool invariant, six gradients within 1e-5 relative L-inf; and the
from-image path (check_from_image)."""
import functools

import numpy as np
import pytest
import torch

import far
from util import capture_forward_args, check_backward, check_forward, check_from_image, run_both, to_dev

pytestmark = pytest.mark.gpu

CASES = {"inside": (64, 48, 3), "crowd": (64, 48, 16)}        # frame W, H and lattice half-width n
TEMPS = [1.0, 0.5, 0.0]


def _C():
    from dmesh2_renderer_amd import _C as c
    return c


def _nthreads():
    from oracle import cpu as orc
    return min(orc.max_threads(), 16)


class _flags:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.old = _C().set_flags(self.flags)

    def __exit__(self, *exc):
        _C().set_flags(self.old)


@functools.lru_cache(maxsize=None)
def _scene(case):
    W, H, n = CASES[case]
    return far.inside_scene(W, H, 5, n=n)


@functools.lru_cache(maxsize=None)
def _args(case, prep, temp):
    """The 21 boundary arguments (CPU tensors) the module hands the op for ``case``: the fused prep runs on the GPU."""
    sc = _scene(case)
    args, r = capture_forward_args(sc, [0], [[0, 0]], sc.width, sc.height, temp, 20, device="cuda" if prep == "fused" else "cpu")
    assert prep != "fused" or r.fused_prep
    return tuple(a.cpu() if torch.is_tensor(a) else a for a in args)


@pytest.mark.parametrize("prep", ["fused", "torch"])
@pytest.mark.parametrize("case", list(CASES))
def test_offscreen_scene_content(case, prep):
    """The scene really holds what it is for: binned faces with |verts_image| > 1e5 px, clamped |w|, binned faces with a vertex
    behind the camera, binned faces whose bounding box covers the whole frame."""
    from oracle import cpu as orc
    sc = _scene(case)
    args = _args(case, prep, 1.0)
    W, H = sc.width, sc.height
    vi, ndc, fc = args[9].numpy(), args[8].numpy(), args[5].numpy().astype(np.int64)
    w = far.clip_w(sc.verts.numpy(), sc.mv.numpy(), sc.proj.numpy())[0]
    binned = orc.Binning(1, vi.shape[1], fc.shape[0], W, H, args[1].numpy(), fc, ndc, vi).tiles_touched > 0
    fv = vi[0][fc]
    clamped = np.abs(w) < 1e-4
    assert clamped.sum() >= 40 and (np.abs(ndc[0, clamped, 2]) > 1e4).all()          # (clip z / +-1e-4)
    assert (binned & (np.abs(fv).max(axis=(1, 2)) > 1e5)).sum() >= 100
    assert (binned & clamped[fc].any(axis=1)).sum() >= 100
    assert (binned & (w[fc] < 0).any(axis=1)).sum() >= 100
    spans = (fv[..., 0].min(1) <= 0) & (fv[..., 0].max(1) >= W) & (fv[..., 1].min(1) <= 0) & (fv[..., 1].max(1) >= H)
    assert (binned & spans).sum() >= 100


def _want_mode(case, temp, kernels):
    C = _C()
    if kernels == "legacy":
        return C.FWD_NONE
    if temp == 0.0:
        return C.FWD_POINT
    return C.FWD_MASKS if case == "crowd" else C.FWD_POOL


@pytest.mark.parametrize("kernels", ["dense", "legacy"])
@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("prep", ["fused", "torch"])
@pytest.mark.parametrize("case", list(CASES))
def test_offscreen_parity(case, prep, temp, kernels):
    """Materialised tables: forward bit-exact (the pool invariant included), six gradients within 1e-5, both kernel families;
    the forward mode each run took is the one this frame's pair bound calls for."""
    C = _C()
    args = list(_args(case, prep, temp))
    with _flags(C.DM2_FLAG_LEGACY_KERNELS if kernels == "legacy" else 0):
        res = run_both(args, seed=int(10 * temp) + 1, nthreads=_nthreads())
        mode = C.last_forward_mode()
    check_forward(res, args)
    worst = check_backward(res)
    print(f"\n{case} {prep} t{temp} {kernels}: forward mode {mode}, " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert mode == _want_mode(case, temp, kernels), mode


@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("case", list(CASES))
def test_offscreen_from_image(case, temp):
    """The default op path (bench.py's): tables built from verts_image in the plan, the AA gradient routed to the vertices."""
    C = _C()
    args = to_dev(list(_args(case, "fused", temp)))
    g = torch.Generator().manual_seed(12)
    B, ph, pw = args[9].shape[0], int(args[3]), int(args[2])
    wc = torch.randn((B, ph, pw, 3), generator=g).cuda(); wd = torch.randn((B, ph, pw), generator=g).cuda()
    worst = check_from_image(args, wc, wd, nthreads=_nthreads())
    mode = C.last_forward_mode()
    print(f"\n{case} t{temp} from-image: forward mode {mode}, " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert mode == _want_mode(case, temp, "dense"), mode
