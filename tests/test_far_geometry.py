"""The far off-screen generators (tests/far.py) hold what the GPU tests rely on -- checked on the CPU, with the oracle and numpy
only: corners ~reach px from the tested pixel, exact far-magnitude ties (long edges through a pixel corner, near corners on a
pixel line), nearly axis-parallel long edges, and a camera-inside lattice with clamped |w|, vertices behind the camera and
binned faces 1e5 px across that cover the whole frame."""
import numpy as np
import pytest

import far
import structured as S
from util import capture_forward_args


@pytest.mark.parametrize("reach", far.REACHES)
def test_far_pairs_properties(reach):
    from oracle import cpu as orc
    tris, pms, kind = far.far_pairs(int(np.log10(reach)) * 1000 + 7, 10000, reach)      # (test_gpu_clippers.py's sets)
    c = pms.astype(np.float64) + 0.5
    dist = np.linalg.norm(tris.astype(np.float64) - c[:, None, :], axis=-1)            # (n,3) corner -> pixel centre
    ndist = np.sort(dist, axis=1)
    assert (ndist[:, 0] <= 8).all()                                                     # a corner next to the pixel
    assert (ndist[:, 2] >= 0.6 * reach).all()                                           # and one ~reach away
    assert (tris < 0).any(axis=(1, 2)).mean() >= 0.1                                    # negative coordinates
    for base in far.BASES:
        assert ((pms >= base) & (pms < base + 16)).all(axis=1).sum() >= 2500
    t = orc.aa_tables(tris, np.float32, reorder=True)
    tie = S.exact_ties(t["verts"], pms)
    k = lambda name: kind == far.KINDS.index(name)
    # the corner construction: an edge through a pixel corner exactly, where its far end was not moved off
    assert tie[k("corner")].mean() >= 0.4, tie[k("corner")].mean()
    # the line construction: a corner exactly on a pixel line (the others are 1 ulp off it)
    assert tie[k("line")].mean() >= 0.4, tie[k("line")].mean()
    assert tie[k("wedge") | k("sliver")].mean() <= 0.01
    # the axis construction: long edges whose short component is 0, inside "iszero", or up to 2 px
    e = np.abs(t["edges"].astype(np.float64))[k("axis")]
    short, long = e.min(axis=-1), e.max(axis=-1)
    axial = long >= 0.5 * reach
    assert (axial & (short == 0)).any(axis=1).sum() >= 100
    assert (axial & (short > 0) & (short < 1e-3)).any(axis=1).sum() >= 100
    assert (axial & (short >= 1e-3) & (short < 1 / 64)).any(axis=1).sum() >= 100


def test_inside_scene_properties():
    """The camera-inside lattice of tests/test_gpu_offscreen.py ("inside"), through the reference-shaped torch prep."""
    from oracle import cpu as orc
    sc = far.inside_scene(64, 48, 5, n=3)
    args, _ = capture_forward_args(sc, [0], [[0, 0]], 64, 48, 1.0, 20)
    vi, ndc, fc = args[9].numpy(), args[8].numpy(), args[5].numpy().astype(np.int64)
    w = far.clip_w(sc.verts.numpy(), sc.mv.numpy(), sc.proj.numpy())[0]
    clamped = np.abs(w) < 1e-4
    assert clamped.sum() == 49 and (np.abs(ndc[0, clamped, 2]) > 1e4).all()
    binned = orc.Binning(1, vi.shape[1], fc.shape[0], 64, 48, args[1].numpy(), fc, ndc, vi).tiles_touched > 0
    fv = vi[0][fc]
    assert (binned & (np.abs(fv).max(axis=(1, 2)) > 1e5)).sum() >= 200
    assert (binned & clamped[fc].any(axis=1)).sum() >= 200
    assert (binned & (w[fc] < 0).any(axis=1)).sum() >= 200
    spans = (fv[..., 0].min(1) <= 0) & (fv[..., 0].max(1) >= 64) & (fv[..., 1].min(1) <= 0) & (fv[..., 1].max(1) >= 48)
    assert (binned & spans).sum() >= 150
