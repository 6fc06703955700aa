"""The structured scenes (tests/structured.py) have the properties tests/test_gpu_structured.py relies on -- checked on the
CPU, with the oracle and numpy only: corners exactly on the intended lattice, "iszero" edges in the tables, pairs on which the
reference raises, and a floor of (pixel, face) pairs that are exact geometric ties (a corner on one of the pixel's lines, an
edge through one of its corners).  A soup has almost none of the last (checked too, as the contrast)."""
import numpy as np
import pytest

import structured as S
from util import from_image_oracle_args, scenes, soup_args

# per scene: exact-tie share of the live pairs, "iszero" table entries, oracle error-coded pairs -- floors a little under what
# the generators produce (0.66 / 0.25 / 0.27 / 0.40 / 0.84 / 0.26 of the live pairs are exact ties)
FLOORS = {
    "grid": dict(tie=0.55, iszero=6000, errors=15000),
    "subpixel": dict(tie=0.2, iszero=500, errors=2000),
    "iszero": dict(tie=0.2, iszero=800, errors=3000),
    "large": dict(tie=0.3, iszero=10000, errors=15000),
    "degenerate": dict(tie=0.7, iszero=800, errors=4000),
    "coplanar": dict(tie=0.2, iszero=3000, errors=8000),
    "far": dict(tie=0.09, iszero=800, errors=5000),              # (0.11 exact ties, mostly the backdrop's)
}


def _pairs(args):
    b, f, pm = S.bbox_pairs(args)
    area, _, code = S.oracle_pairs(args, b, f, pm)
    live = (code == 0) & (area != 0)
    tie = S.exact_ties(args[12].numpy()[b, f], pm)
    return b, f, pm, area, code, live, tie


@pytest.mark.parametrize("name", S.EXACT)
def test_scene_properties(name):
    args = S.make_args(name)
    g = S._geometry(name)
    vi = args[9].numpy()
    # verts_image is the intended geometry in fp32, for every view, and (but for the iszero scene) on its lattice
    assert all(np.array_equal(vi[b], g["xy"].astype(np.float32)) for b in range(vi.shape[0]))
    step = S.LATTICE.get(name)
    if step is not None:
        lat = vi[:, :g["nlat"]]
        assert np.array_equal(np.floor(lat / step) * step, lat)
    # the tables are the reference's, built from the snapped verts_image (CCW reorder included)
    na = from_image_oracle_args(args)
    for k in range(12, 18):
        assert np.array_equal(np.asarray(na[k]), args[k].numpy()), k
    fl = FLOORS[name]
    assert int(args[14].numpy().sum()) >= fl["iszero"]
    b, f, pm, area, code, live, tie = _pairs(args)
    assert int((code != 0).sum()) >= fl["errors"]                            # the "reference raises" skip path is present
    assert live.sum() >= 1000
    assert tie[live].mean() >= fl["tie"], tie[live].mean()
    if name == "iszero":
        # edge components exactly 0, within (0, 1e-3) and just above 1e-3 (the tables' own fp32 edges)
        e = np.abs(args[13].numpy()).reshape(-1)
        assert (e == 0).sum() >= 100 and ((e > 0) & (e < 1e-3)).sum() >= 200 and ((e >= 1e-3) & (e < 1.6e-3)).sum() >= 100
    if name == "large":
        assert vi.shape[0] == 2 and (vi[..., 0] >= 3690).all() and (vi[..., 1] >= 1990).all() and (args[1].numpy() >= [3700, 2000]).all()
    if name == "far":
        # corners far outside the 64 x 48 frame in every direction, the faces binned in the frame (bbox pairs), few pairs
        W, H = g["W"], g["H"]
        out = np.maximum(np.maximum(-vi[0, :, 0], vi[0, :, 0] - W), np.maximum(-vi[0, :, 1], vi[0, :, 1] - H))
        assert (out > 5e3).sum() >= 150 and (out > 1e5).sum() >= 150 and (out > 5e6).sum() >= 60
        x, y = vi[0, :, 0], vi[0, :, 1]
        for side in (x < -1e5, x > W + 1e5, y < -1e5, y > H + 1e5):          # past every side of the frame
            assert side.sum() >= 20
        assert len(b) <= 150_000
        assert len(np.unique(f[live & (out[args[5].numpy()[f]].max(axis=1) > 1e5)])) >= 100
    if name == "degenerate":
        v = args[12].numpy()
        a2 = (v[..., 1, 0] - v[..., 0, 0]) * (v[..., 2, 1] - v[..., 0, 1]) - (v[..., 2, 0] - v[..., 0, 0]) * (v[..., 1, 1] - v[..., 0, 1])
        assert (a2 == 0).sum() >= 300                                         # zero-area faces
    if name == "coplanar":
        fc = args[5].numpy()
        F = fc.shape[0] // 3
        assert np.array_equal(fc[:F], fc[F:2 * F]) and np.array_equal(fc[:F][:, [0, 2, 1]], fc[2 * F:])
        z = args[8].numpy()[0, :, 2]
        assert np.array_equal(z[fc[:F]], z[fc[2 * F:][:, [0, 2, 1]]])        # equal depths, hence equal sort keys


def test_projected_scene_is_near_the_lattice():
    """The un-snapped scene: its prep puts the corners within a few ulp of the lattice, mostly not on it."""
    args = S.make_args("projected")
    vi = args[9].numpy()[0].astype(np.float64)
    xy = S._geometry("projected")["xy"]
    dev = np.abs(vi - xy)
    assert dev.max() <= 8 * np.spacing(np.float32(64.0)) and (dev > 0).mean() >= 0.3


def test_soup_has_few_exact_ties():
    args, _ = soup_args(56, 50, 1500, scenes.SEED_BASE + 99)
    b, f, pm, area, code, live, tie = _pairs(args)
    assert tie[live].mean() <= 0.01, tie[live].mean()
