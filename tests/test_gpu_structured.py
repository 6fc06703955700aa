"""GPU parity on pixel-aligned and degenerate geometry (tests/structured.py): watertight pixel grids, the quarter-pixel lattice,
near-"iszero" edges, 4K coordinates, zero-area faces, coplanar duplicates, and a projected (un-snapped) grid within a few ulp
of the lattice.  On these most live (pixel, face) pairs are ties of the default backward's polygon-free Jacobian
(dm2_clip_fast.h), so the tie queue, k_aa_ties and the segment clipper carry a frame's AA gradient, and the temperature-0
forward's quick test meets pixel-centre rays that lie on edges within rounding.

Bars, as in test_gpu_parity.py: forward outputs and integer state bit-exact, the pool invariant, all six gradients within
GRAD_TOL = 1e-5 relative L-inf with the same non-finite pattern, the routed AA gradient within 1e-5 of the fp64 scatter."""
import functools

import numpy as np
import pytest
import torch

import structured as S
from util import (GRAD_TOL, check_backward, check_forward, check_from_image, check_pool, pool_state, rel_linf,
                  run_both, to_dev, to_numpy_args)

pytestmark = pytest.mark.gpu

TEMP_K = [(1.0, 20), (1.0, 0), (0.5, 20), (0.5, 0), (0.0, 20), (0.0, 0)]


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


def _report(what, worst):
    print(f"\n{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("kernels", ["dense", "legacy"])
@pytest.mark.parametrize("temp,K", TEMP_K, ids=[f"t{t}-K{k}" for t, k in TEMP_K])
@pytest.mark.parametrize("name", S.ALL)
def test_structured_parity(name, temp, K, kernels):
    """Materialised tables: forward bit-exact, six gradients within 1e-5, both kernel families."""
    args = S.make_args(name, temp, K)
    with _flags(_C().DM2_FLAG_LEGACY_KERNELS if kernels == "legacy" else 0):
        res = run_both(args, seed=K + int(10 * temp), nthreads=_nthreads())
    check_forward(res, args)
    _report(f"{name} t{temp} K{K} {kernels}", check_backward(res))


@pytest.mark.parametrize("temp", [1.0, 0.5])
@pytest.mark.parametrize("name", S.ALL)
def test_structured_masks_only(name, temp):
    """The masks-only backward (no pair pool): every pair is re-clipped by the segment clipper."""
    args = S.make_args(name, temp, 20)
    with _flags(_C().DM2_FLAG_NO_PAIR_POOL):
        res = run_both(args, seed=3, nthreads=_nthreads())
        assert _C().last_forward_mode() != _C().FWD_POOL
    check_forward(res, args)
    _report(f"{name} t{temp} masks-only", check_backward(res))


@pytest.mark.parametrize("temp", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("name", S.ALL)
def test_structured_from_image(name, temp):
    """The default op path (bench.py's): tables built from verts_image in the plan, the AA gradient routed to the vertices."""
    args = to_dev(S.make_args(name, temp, 20))
    g = torch.Generator().manual_seed(11)
    B, ph, pw = args[9].shape[0], int(args[3]), int(args[2])
    wc = torch.randn((B, ph, pw, 3), generator=g).cuda(); wd = torch.randn((B, ph, pw), generator=g).cuda()
    _report(f"{name} t{temp} from-image", check_from_image(args, wc, wd, tol=GRAD_TOL, nthreads=_nthreads()))


@pytest.mark.parametrize("name", S.ALL)
def test_structured_backward_twice(name):
    """Two backwards of one forward: the tie queue is emptied by the last block of k_aa_ties, so the second backward sees
    only its own ties and both match the oracle (and each other to summation order)."""
    from oracle import cpu as orc
    C = _C()
    args = S.make_args(name, 1.0, 20)
    dargs = to_dev(args)
    out = C.render_forward_cuda(*dargs)
    check_pool(pool_state(out))
    ref = orc.render_forward_cuda(*to_numpy_args(args), nthreads=_nthreads())
    rng = np.random.RandomState(5)
    gc = rng.randn(*ref.color.shape).astype(np.float32); gd = rng.randn(*ref.depth.shape).astype(np.float32)
    gref = orc.render_backward_cuda(ref, gc, gd, nthreads=_nthreads())
    bw = (out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(), out[7], out[8], out[9], out[3], out[4], out[5], out[6])
    runs = []
    for _ in range(2):
        runs.append([x.cpu().numpy() for x in C.render_backward_cuda(*bw)])
    torch.cuda.synchronize()
    for grads in runs:
        check_backward(dict(grads=grads, ref_grads=gref))
    for a, b in zip(*runs):
        m = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), m) and rel_linf(a[m], b[m]) <= GRAD_TOL


@pytest.mark.parametrize("temp", [1.0, 0.0])
@pytest.mark.parametrize("name", ["grid", "degenerate"])
def test_structured_analytic_rays(name, temp):
    """Rays computed per pixel by the kernels (DM2_FLAG_ANALYTIC_RAYS) against the oracle fed with the same closed form."""
    from oracle import cpu as orc
    C = _C()
    args = list(S.make_args(name, temp, 20))
    sc, geo = S.scene(name)
    B = args[9].shape[0]
    cam = torch.cat((torch.inverse(sc.mv).reshape(-1, 16), torch.inverse(sc.proj).reshape(-1, 16)), dim=1).float().contiguous()
    ro, rd = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4).numpy(), cam[:, 16:].reshape(-1, 4, 4).numpy(),
                                            geo["W"], geo["H"])
    pm, pw, ph = args[1].numpy(), int(args[2]), int(args[3])
    cut = lambda r: torch.from_numpy(np.stack([r[b, pm[b, 1]:pm[b, 1] + ph, pm[b, 0]:pm[b, 0] + pw] for b in range(B)]))
    ref_args = list(args); ref_args[19], ref_args[20] = cut(ro), cut(rd)
    dargs = to_dev(args)
    dargs[19] = dargs[20] = torch.empty((B, 0, 0, 3), dtype=torch.float32, device="cuda")
    with C.analytic_rays(cam.cuda(), geo["W"], geo["H"]):
        out = C.render_forward_cuda(*dargs)
        pool = pool_state(out)
        ref = orc.render_forward_cuda(*to_numpy_args(ref_args), nthreads=_nthreads())
        rng = np.random.RandomState(8)
        gc = rng.randn(*ref.color.shape).astype(np.float32); gd = rng.randn(*ref.depth.shape).astype(np.float32)
        grads = C.render_backward_cuda(out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(),
                                       out[7], out[8], out[9], out[3], out[4], out[5], out[6])
        res = dict(out=out, pool=pool, ref=ref, grads=[g.cpu().numpy() for g in grads],
                   ref_grads=orc.render_backward_cuda(ref, gc, gd, nthreads=_nthreads()))
    check_forward(res, ref_args)
    _report(f"{name} t{temp} analytic rays", check_backward(res))


@functools.lru_cache(maxsize=None)
def _fast_pairs(name):
    """The polygon-free clipper (debug variant 4, the default backward's) and the oracle on the scene's bounding-box pairs."""
    C = _C()
    args = S.make_args(name)
    b, f, pm = S.bbox_pairs(args)
    t = S.pair_tables(args, b, f)
    dev = [torch.from_numpy(t[k]).cuda() for k in ("verts", "edges", "iszero", "recip", "normal", "normal_c")]
    area, grad, code = C.debug_aa_overlap(4, *dev, torch.from_numpy(pm).cuda())
    torch.cuda.synchronize()
    o_area, o_grad, o_code = S.oracle_pairs(args, b, f, pm)
    err = np.abs(grad.cpu().numpy() - o_grad).reshape(len(b), -1).max(axis=1) \
        / np.maximum(1.0, np.abs(o_grad).reshape(len(b), -1).max(axis=1))
    return area.cpu().numpy(), code.cpu().numpy(), err, o_area, o_code


@pytest.mark.parametrize("name", S.ALL)
def test_structured_tie_share(name):
    """How much of each scene the default backward hands to the tie path: code -1 of the polygon-free clipper over the scene's
    bounding-box pairs.  Its errors are exactly where the oracle raises, its area is the oracle's on every live pair."""
    area, code, err, o_area, o_code = _fast_pairs(name)
    assert np.array_equal(code > 0, o_code != 0)
    live = (o_code == 0) & (o_area != 0)
    assert np.array_equal(area[live].view(np.uint32), o_area[live].view(np.uint32))
    tie = code == -1
    ok = live & ~tie
    print(f"\n{name}: {len(code)} bbox pairs, {int((o_code != 0).sum())} error-coded by the oracle, {int(live.sum())} live, "
          f"tie share of live {tie[live].mean():.1%}, worst Jacobian error of the other live pairs {err[ok].max() if ok.any() else 0:.2e}")


@pytest.mark.parametrize("name", S.ALL)
def test_structured_fast_jacobian_unflagged_pairs(name):
    """Every live pair the default backward does NOT hand to the tie path has the oracle's Jacobian to 1e-5 of max(1, largest
    entry) (FAST_GRAD_TOL of test_gpu_clippers.py) -- here also the pairs of nearly axis-parallel edges that straddle a pixel
    line (|e| just above the 1e-3 "iszero" threshold), whose crossing's Jacobian is ill-conditioned: tie rule (b) flags them."""
    area, code, err, o_area, o_code = _fast_pairs(name)
    ok = (o_code == 0) & (o_area != 0) & (code != -1)
    assert ok.sum() == 0 or err[ok].max() <= 1e-5, err[ok].max()
