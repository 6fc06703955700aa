"""The reference is defined on every edge scene it is compared on (tests/reference_scenes.py), and every scene still reaches
the branch it exists for -- no GPU, the arguments and the oracle's forward only.

For every scene: reference_lib.races_in_binning is false for every (view, face) (no face is dropped by the z test while it
has a tile rectangle, so nothing had to be removed and no z clamped), verts_ndc and verts_image are finite and every tile
coordinate converts to int (reference_lib.undefined_tile_rects), and the scene's own presence check holds.  This is a
condition, not a measurement: a scene that breaks it is fixed or left out of SCENES by name with the reason, never silently
narrowed."""
import functools

import numpy as np
import pytest

import reference_lib as RL
import reference_scenes as RS
from util import GRAD_TOL, to_numpy_args


@functools.lru_cache(maxsize=None)
def _forward(name):
    from oracle import cpu as orc
    with np.errstate(all="ignore"):
        return orc.render_forward_cuda(*to_numpy_args(RS.args(name)), nthreads=min(orc.max_threads(), 16))


def test_the_scene_list_is_the_one_agreed():
    n = {f: len(RS.names(f)) for f in RS.FAMILIES}
    assert n == {"structured": 11, "tiequeue": 5, "replay": 12, "camera": 3, "desync": 2}, n
    assert set(RS.names("structured")) >= {"structured/grid_t1", "structured/grid_t05", "structured/grid_t0", "structured/iszero_t05",
                                           "structured/large_t1", "structured/far_t1", "structured/projected_t1"}


@pytest.mark.parametrize("name", RS.names())
def test_reference_is_defined_and_feature_present(name):
    sc = RS.SCENES[name]
    a = RS.args(name)
    n = to_numpy_args(a)
    assert float(n[11]) == sc.temp
    ndc, img, pm = n[8], n[9], n[1]
    assert np.isfinite(ndc).all() and np.isfinite(img).all()
    assert RL.undefined_tile_rects(ndc, img, pm) is None
    raced = RL.races_in_binning(n[5], ndc, img, pm, int(n[2]), int(n[3]))
    assert raced.shape == (ndc.shape[0], n[5].shape[0])
    RL._defined(n[5], ndc, img, pm, int(n[2]), int(n[3]))                       # what the loader asks before every call
    ref = _forward(name)
    sc.present(a, ref)
    print(f"\n[reference scenes] {name}: {ndc.shape[0]} views, {n[5].shape[0]} faces, {int(n[2])} x {int(n[3])} px, "
          f"{int(raced.sum())} raced faces, num_rendered {ref.num_rendered}, feature present")
    assert not raced.any()


def test_desync_corner_is_real_in_the_oracle():
    """K does not reach the image; the oracle's K = 20 gradients leave its K = 0 gradients by more than 1e-3."""
    from oracle import cpu as orc
    from util import GRAD_NAMES, rel_linf
    r20, r0 = _forward("desync/k20"), _forward("desync/k0")
    assert np.array_equal(r20.color, r0.color) and np.array_equal(r20.n_contrib, r0.n_contrib)
    rng = np.random.RandomState(3)
    gc, gd = rng.randn(*r20.color.shape).astype(np.float32), rng.randn(*r20.depth.shape).astype(np.float32)
    g20, g0 = orc.render_backward_cuda(r20, gc, gd), orc.render_backward_cuda(r0, gc, gd)
    assert max(rel_linf(g20[k], g0[k]) for k in GRAD_NAMES) > 1e-3


@pytest.mark.parametrize("what", ["nan image", "inf ndc z", "tile out of int range", "raced face"])
def test_loader_refuses_what_the_reference_does_not_define(what):
    n = to_numpy_args(RS.args("tiequeue/none"))
    fc, ndc, img, pm = n[5], n[8].copy(), n[9].copy(), n[1]
    if what == "nan image":
        img[0, 3, 1] = np.nan
    elif what == "inf ndc z":
        ndc[0, 2, 2] = np.inf
    elif what == "tile out of int range":
        img[0, 5, 0] = 4.0e10
    else:
        ndc[0, fc[0], 2] = 1.5                                                  # dropped by the z test, its rectangle kept
        assert RL.races_in_binning(fc, ndc, img, pm, int(n[2]), int(n[3]))[0, 0]
    with pytest.raises(ValueError, match="reference's binning"):
        RL._defined(fc, ndc, img, pm, int(n[2]), int(n[3]))


def test_slack_view_keeps_values_and_owns_what_the_backward_reads():
    import torch
    for B, H, W in ((1, 16, 16), (2, 44, 56), (1, 24, 40), (3, 72, 96)):
        t = torch.arange(B * H * W, dtype=torch.int32).reshape(B, H, W)
        v = RL._with_slack(t)
        assert v.shape == t.shape and v.is_contiguous() and torch.equal(v, t)
        H16, W16 = -(-H // 16) * 16, -(-W // 16) * 16
        last = (B - 1) * H * W + (H16 - 1) * W + (W16 - 1)                       # the farthest entry a thread of the grid reads
        assert v.untyped_storage().nbytes() // 4 > last


def test_gradient_acceptance_gives_relief_only_for_the_reference_s_own_noise():
    """reference_lib.accept_gradients on made-up numbers: within 1e-5 float64 is never asked; a miss with the reference within
    1e-5 of float64 fails at 1e-5; a reference 4e-5 from float64 widens the bound to 8e-5 against float64, from its own
    distance alone, and what lies farther still fails."""
    truth = {"t": np.array([1.0, -0.5, 0.25])}

    def never():
        raise AssertionError("float64 asked although every tensor was within the bound")

    off = lambda e: {"t": truth["t"] + np.array([0.0, e, 0.0])}                # noqa: E731
    fig, wide, fail = RL.accept_gradients(off(0.0), {"a": off(5e-6)}, never, GRAD_TOL)
    assert not wide and not fail and fig["t"]["vs_ref"]["a"] == pytest.approx(5e-6)
    fig, wide, fail = RL.accept_gradients(off(2e-6), {"a": off(2e-5)}, lambda: truth, GRAD_TOL)
    assert not wide and [f[:2] for f in fail] == [("t", "a")] and fail[0][3] == GRAD_TOL
    fig, wide, fail = RL.accept_gradients(off(4e-5), {"a": off(-3e-5), "b": off(-9e-5)}, lambda: truth, GRAD_TOL)
    assert wide == ["t"] and fig["t"]["bound"] == pytest.approx(8e-5)
    assert [f[:2] for f in fail] == [("t", "b")]


def test_every_pixel_centre_of_the_grid_lies_on_an_edge():
    """What tests/test_gpu_reference_edges.py::test_shipped_variant_lattice_scene_rays_off_the_edges starts from; a soup frame
    has no such pixel."""
    assert RS.centres_on_edges(RS.args("structured/grid_t1")).all()
    assert not RS.centres_on_edges(RS.args("tiequeue/none")).any()
