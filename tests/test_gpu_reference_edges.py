"""The oracle and the HIP kernels held to the reference's own kernels (oracle/build_ref.py, tests/reference_lib.py) on the
suite's edge scenes (tests/reference_scenes.py; tests/test_reference_scenes_cpu.py shows that the reference is defined on
every one of them): pixel-aligned, sub-pixel, "iszero", 4K, degenerate, coplanar, far and projected geometry, the tie queue's
lattices, the backward replay's stacks and opaque faces, general cameras, and the record stack's desync corner.

  forward   strict reference == oracle bit for bit on everything tests/test_gpu_reference.py compares; HIP kernels in both
            work distributions == strict reference bit for bit: num_rendered, colour, raw depth;
  backward  the strict reference's backward on its own forward's buffers against the oracle and against the kernels on every
            route the scene's temperature has -- default (pair pool / point), DM2_FLAG_NO_PAIR_POOL (masks),
            DM2_FLAG_LEGACY_KERNELS -- each with its last_forward_mode() asserted; on the structured scenes also the
            tables-from-image path bench.py times.  Acceptance per tensor: reference_lib.accept_gradients;
  desync    the corner of DESIGN.md §6 asked of the reference itself: its K = 20 gradients leave its own K = 0 gradients,
            the oracle follows it in both, the kernels equal its K = 0 path on the K = 20 arguments;
  shipped   tests/test_gpu_reference.py's shipped-variant procedure on the pixel lattice.

Every test skips only where the reference modules were not built (reference_lib.load() is None).
"""
import functools

import numpy as np
import pytest
import torch

import reference_lib as RL
import reference_scenes as RS
from util import (GRAD_NAMES, GRAD_TOL, _C, from_image_oracle_args, rel_linf, run_from_image, scatter_aa_grad_to_verts,
                  to_numpy_args)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_EXCLUDED = 0.01            # tests/test_gpu_reference.py's cap on the pixels whose integer records differ between the builds
ROUTES = {                     # flags, and the forward mode that route must report at temperature > 0 / == 0 (None: not run)
    "default": (0, "FWD_POOL", "FWD_POINT"),
    "masks": (_C.DM2_FLAG_NO_PAIR_POOL, "FWD_MASKS", None),
    "legacy": (_C.DM2_FLAG_LEGACY_KERNELS, "FWD_NONE", "FWD_NONE"),
}


def _ref(variant="strict"):
    mod = RL.load(variant)
    if mod is None:
        pytest.skip("oracle/_ref/ holds no reference build")
    return mod


def _threads():
    from oracle import cpu as orc
    return min(orc.max_threads(), 16)


@functools.lru_cache(maxsize=None)
def _oracle_forward(name):
    """The oracle's forward of scene ``name``: computed once, read-only."""
    from oracle import cpu as orc
    with np.errstate(all="ignore"):
        return orc.render_forward_cuda(*to_numpy_args(RS.args(name)), nthreads=_threads())


@functools.lru_cache(maxsize=None)
def _ref_forward(name):
    """The strict reference's forward of scene ``name``: run once, read-only (its backward only reads the buffers)."""
    return RL.Forward(_ref(), RL.to_device(RS.args(name), DEV))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    n = int((_bits(a) != _bits(b)).sum())
    assert n == 0, f"{what}: {n} of {a.size} entries differ"


class _flags:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.old = _C.set_flags(self.flags)

    def __exit__(self, *exc):
        _C.set_flags(self.old)


def _seeded_grads(shape_c, shape_d, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(*shape_c).astype(np.float32), rng.randn(*shape_d).astype(np.float32)


# ---- forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RS.names())
def test_forward_reference_equals_oracle(name):
    ref, orc = _ref_forward(name), _oracle_forward(name)
    assert ref.num_rendered == orc.num_rendered > 0
    _same(ref.color, orc.color, "colour")
    _same(ref.depth, orc.depth, "depth")
    _same(ref.tri_cnt, orc.buf_tri_cnt, "tri_cnt")
    _same(ref.tri_id, orc.buf_tri_id, "tri_id")
    _same(ref.oarea, orc.buf_oarea, "oarea")
    _same(ref.doarea, orc.buf_doarea, "doarea")
    _same(ref.image["final_T"], orc.final_T, "final_T")
    _same(ref.image["final_prev_T"], orc.final_prev_T, "final_prev_T")
    _same(ref.image["n_contrib"], orc.n_contrib, "n_contrib")
    _same(ref.image["ranges"], orc.binning.ranges, "ranges")
    _same(ref.face_list, orc.binning.face_list, "face_list")


@pytest.mark.parametrize("legacy", [False, True], ids=["default", "legacy"])
@pytest.mark.parametrize("name", RS.names())
def test_forward_kernels_equal_reference(name, legacy):
    ref = _ref_forward(name)
    with _flags(_C.DM2_FLAG_LEGACY_KERNELS if legacy else 0):
        out = _C.render_forward_cuda(*ref.dargs)
        torch.cuda.synchronize()
    assert out[0] == ref.num_rendered
    _same(out[1].cpu().numpy(), ref.color, "colour")
    _same(out[2].cpu().numpy(), ref.depth, "raw depth")


# ---- backward --------------------------------------------------------------------------------------------------------------
def _kernels_backward(dargs, dgc, dgd, temp, route):
    """The HIP kernels' forward + backward under ``route`` -> the six gradients (numpy); the route's forward mode asserted."""
    flags, mode_aa, mode_point = ROUTES[route]
    with _flags(flags):
        out = _C.render_forward_cuda(*dargs)
        mode = _C.last_forward_mode()
        g = [x.cpu().numpy() for x in _C.render_backward_cuda(out[0], *dargs, dgc, dgd, out[7], out[8], out[9], out[3], out[4],
                                                              out[5], out[6])]
        torch.cuda.synchronize()
    assert mode == getattr(_C, mode_aa if temp > 0 else mode_point), (route, mode)
    return dict(zip(GRAD_NAMES, g))


def _f64_gradients(name, gc, gd):
    def run():
        from oracle import cpu as orc
        with np.errstate(all="ignore"):
            r64 = orc.render_forward_cuda(*to_numpy_args(RS.args(name)), dtype=np.float64, nthreads=_threads())
            return orc.render_backward_cuda(r64, gc.astype(np.float64), gd.astype(np.float64), nthreads=_threads())
    return run


@functools.lru_cache(maxsize=None)
def _reference_backward(name, seed):
    """-> (gc, gd, the strict reference's six gradients on its own forward's buffers, the oracle's), computed once."""
    from oracle import cpu as orc
    ref = _ref_forward(name)
    gc, gd = _seeded_grads(ref.color.shape, ref.depth.shape, seed)
    g = RL.backward(_ref(), ref, torch.from_numpy(gc).to(DEV), torch.from_numpy(gd).to(DEV))
    for nm, x in zip(GRAD_NAMES, g):
        assert np.isfinite(x).all(), nm
    with np.errstate(all="ignore"):
        g_orc = orc.render_backward_cuda(_oracle_forward(name), gc, gd, nthreads=_threads())
    return gc, gd, dict(zip(GRAD_NAMES, g)), {nm: g_orc[nm] for nm in GRAD_NAMES}


def _judge(label, ref, others, f64):
    for who, g in others.items():
        for nm in ref:
            assert g[nm].shape == ref[nm].shape, (who, nm)
    figures, widened, failures = RL.accept_gradients(ref, others, f64, GRAD_TOL)
    print(f"\n[reference backward] {label}: rel L-inf ({', '.join(others)}) " + RL.describe(figures))
    for nm in widened:
        print(f"[reference backward] WIDENED {label} {nm}: reference vs float64 {figures[nm]['ref_vs_f64']:.3e}, bound "
              f"{figures[nm]['bound']:.3e}, vs float64 {figures[nm]['vs_f64']}")
    assert any(np.abs(g).max() > 0 for g in ref.values())
    assert not failures, failures


def _seed(name):
    return 5 if RS.SCENES[name].family == "desync" else len(name)        # (both desync scenes: the same output gradients)


@pytest.mark.parametrize("name", RS.names())
def test_backward_reference_against_oracle_and_every_route(name):
    """desync/k20 holds the oracle alone: there the kernels equal the reference's K = 0 path by design, which
    test_desync_corner_in_the_reference asserts on the same arguments."""
    temp = RS.SCENES[name].temp
    gc, gd, g_ref, g_orc = _reference_backward(name, _seed(name))
    others = {"oracle": g_orc}
    if name != "desync/k20":
        dargs = _ref_forward(name).dargs
        dgc, dgd = torch.from_numpy(gc).to(DEV), torch.from_numpy(gd).to(DEV)
        for route, (_, _, mode_point) in ROUTES.items():
            if temp > 0 or mode_point is not None:
                others[route] = _kernels_backward(dargs, dgc, dgd, temp, route)
                assert not others[route]["verts_ndc"][..., :2].any()
    _judge(name, g_ref, others, _f64_gradients(name, gc, gd))


@pytest.mark.parametrize("name", RS.names("structured"))
def test_backward_from_image_path_against_reference(name):
    """The path bench.py times: placeholder tables, the tables built from verts_image in the plan, the AA gradient routed to
    the vertices.  The scene's tables ARE the ones the reference builds from its verts_image (asserted), so the reference's
    run on the scene's arguments is the reference of this path; its AA gradient gets the same scatter (fp64)."""
    a = RS.args(name)
    na = from_image_oracle_args(a)
    for k in range(12, 18):
        assert np.array_equal(np.asarray(na[k]), a[k].numpy()), k
    gc, gd, g_ref, _ = _reference_backward(name, _seed(name))
    ref = _ref_forward(name)

    def routed(g):
        return dict(g, aa_to_verts=scatter_aa_grad_to_verts(g["aa_face_verts"], na[12], na[9], na[5]))

    with _flags(0):
        out, g, g_routed, _ = run_from_image(ref.dargs, torch.from_numpy(gc).to(DEV), torch.from_numpy(gd).to(DEV))
    assert out[0] == ref.num_rendered
    _same(out[1].cpu().numpy(), ref.color, "colour")
    _same(out[2].cpu().numpy(), ref.depth, "raw depth")
    _same(out[5].cpu().numpy(), ref.tri_cnt, "tri_cnt")
    got = dict(zip(GRAD_NAMES, g), aa_to_verts=g_routed)
    f64 = _f64_gradients(name, gc, gd)
    _judge(name + " from image", routed(g_ref), {"from image": got}, lambda: routed(f64()))


# ---- the desync corner, asked of the reference itself ----------------------------------------------------------------------
def test_desync_corner_in_the_reference():
    """where a record of a face that never blends lies on top of a pixel's stack behind the pixel's last
    contributor, the reference's K > 0 backward never pops it and loses the pixel's AA records; its K = 0 path recomputes.
    The oracle follows the reference on both paths (test_backward_reference_against_oracle_and_every_route on desync/k20 and
    desync/k0); here: K does not reach the reference's image, its K = 20 gradients leave its own K = 0 gradients by more than
    1e-3 on some tensor, and the kernels, on the K = 20 arguments and every route, equal its K = 0 gradients."""
    f20, f0 = _ref_forward("desync/k20"), _ref_forward("desync/k0")
    _same(f20.color, f0.color, "colour")
    _same(f20.depth, f0.depth, "depth")
    _same(f20.image["n_contrib"], f0.image["n_contrib"], "n_contrib")
    assert f20.tri_cnt.max() > 0 and f0.tri_cnt.max() == 0
    gc, gd, g20, _ = _reference_backward("desync/k20", _seed("desync/k20"))
    gc0, gd0, g0, _ = _reference_backward("desync/k0", _seed("desync/k0"))
    assert np.array_equal(gc, gc0) and np.array_equal(gd, gd0)
    dev = {nm: rel_linf(g20[nm], g0[nm]) for nm in GRAD_NAMES}
    lost = int((np.abs(g20["faces_opacity"] - g0["faces_opacity"]) > 1e-6 * np.abs(g0["faces_opacity"]).max()).sum())
    print("\n[reference desync] the reference's K = 20 against its own K = 0 gradients, rel L-inf: "
          + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()) + f"; {lost} of {g0['faces_opacity'].size} opacity gradients differ")
    assert max(dev.values()) > 1e-3                           # the corner is real in the reference, not only in the restatement
    dgc, dgd = torch.from_numpy(gc).to(DEV), torch.from_numpy(gd).to(DEV)
    others = {route: _kernels_backward(f20.dargs, dgc, dgd, 1.0, route) for route in ROUTES}
    _judge("desync: kernels on K = 20 against the reference's K = 0", g0, others, _f64_gradients("desync/k0", gc, gd))


# ---- the shipped variant on the pixel lattice ------------------------------------------------------------------------------
def _shipped_deviation(label, args):
    """tests/test_gpu_reference.py::test_shipped_variant_soup's first half on the 21 arguments ``args``: both reference builds, the
    pixels whose integer records differ, the output gradients zero there, what contraction alone moves on the others."""
    strict, shipped = _ref("strict"), _ref("shipped")
    dargs = RL.to_device(args, DEV)
    fs, fh = RL.Forward(strict, dargs), RL.Forward(shipped, dargs)
    B, H, W = fs.depth.shape
    assert fs.num_rendered == fh.num_rendered
    differ = (fs.tri_cnt != fh.tri_cnt) | (fs.tri_id != fh.tri_id).any(-1) \
        | (fs.image["n_contrib"] != fh.image["n_contrib"]).reshape(B, H, W)
    keep = ~differ
    dev = {"color": rel_linf(fh.color[keep], fs.color[keep]), "depth": rel_linf(fh.depth[keep], fs.depth[keep])}
    gc, gd = _seeded_grads(fs.color.shape, fs.depth.shape, seed=5)
    gc[differ] = 0.0
    gd[differ] = 0.0
    dgc, dgd = torch.from_numpy(gc).to(DEV), torch.from_numpy(gd).to(DEV)
    gs, gh = RL.backward(strict, fs, dgc, dgd), RL.backward(shipped, fh, dgc, dgd)
    for k, nm in enumerate(GRAD_NAMES):
        dev["grad " + nm] = rel_linf(gh[k], gs[k])
    share = float(differ.mean())
    print(f"\n[shipped vs strict] {label}: excluded pixels {int(differ.sum())} of {differ.size} ({share:.4%}); rel L-inf on the "
          "kept pixels: " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    return share, keep, dev, fh, gh, dargs, dgc, dgd


def _kernels_against_shipped(label, keep, dev, fh, gh, dargs, dgc, dgd):
    """The procedure's second half: the kernels against the shipped build on the kept pixels, each tensor within 1e-5 of its
    maximum, or twice the strict-against-shipped deviation ``dev`` where that alone exceeds 1e-5."""
    with _flags(0):
        out = _C.render_forward_cuda(*dargs)
        g = [x.cpu().numpy() for x in _C.render_backward_cuda(out[0], *dargs, dgc, dgd, out[7], out[8], out[9], out[3], out[4],
                                                              out[5], out[6])]
        torch.cuda.synchronize()
    got = {"color": rel_linf(out[1].cpu().numpy()[keep], fh.color[keep]), "depth": rel_linf(out[2].cpu().numpy()[keep], fh.depth[keep])}
    for k, nm in enumerate(GRAD_NAMES):
        got["grad " + nm] = rel_linf(g[k], gh[k])
    tol = {k: (GRAD_TOL if dev[k] <= GRAD_TOL else 2.0 * dev[k]) for k in dev}
    print(f"[kernels vs shipped] {label}: " + ", ".join(f"{k} {v:.3e} (tol {tol[k]:.1e})" for k, v in got.items()))
    assert out[0] == fh.num_rendered
    assert all(got[k] <= tol[k] for k in got), {k: (got[k], tol[k]) for k in got if got[k] > tol[k]}


def test_shipped_variant_lattice_scene():
    """Contraction flips ties, and ties are what the lattice is made of: structured/grid under both reference builds, then the
    kernels against the shipped build on the pixels whose integer records agree, within 1e-5 of each tensor's maximum, or
    twice the strict-against-shipped deviation where that alone exceeds 1e-5.  MAX_EXCLUDED stays the cap: if the grid exceeds
    it, that share is a finding (printed) and the kernel comparison runs on structured/iszero instead.

    Measured: no integer record differs, yet dL/dverts differs by 1.5e-1 of its maximum between the two builds, so this
    test's bound says little about ``verts``; test_shipped_variant_lattice_scene_rays_off_the_edges shows the cause and holds
    ``verts`` at 1e-5."""
    for name in ("structured/grid_t1", "structured/iszero_t1"):
        share, *rest = _shipped_deviation(name, RS.args(name))
        if share <= MAX_EXCLUDED:
            break
        print(f"[shipped vs strict] FINDING: {name} exceeds the cap of {MAX_EXCLUDED:.2%} excluded pixels with {share:.4%}")
    assert share <= MAX_EXCLUDED, f"{name}: {share:.4%} of the pixels differ in their integer records between the two builds"
    _kernels_against_shipped(name, *rest)


RAY_NUDGE = 1e-5               # added to every ray direction's x (0.618 of it to y): some 1e-3 px at the lattice's depths


def test_shipped_variant_lattice_scene_rays_off_the_edges():
    """Why the two reference builds differ by 15 % in dL/dverts on structured/grid although no integer record differs: every
    pixel centre of that scene lies on an edge of some face (reference_scenes.centres_on_edges), so its ray meets faces with u,
    v or 1 - u - v equal to 0 up to rounding, and the one decision the reference takes on (u, v) -- clamp_bary_uv's code
    (auxiliary.h:292-329), which selects clamp_bary_uv_grad's Jacobian, through which only ``verts`` flows -- falls either way
    with contraction.  Shown by moving the rays, and nothing else, off the edges by 1e-5 in direction (far above rounding, far
    below anything that changes a continuous term by more than 1e-5; the image-space tables, hence coverage and every integer
    record's geometry, stay): the deviation of ``verts`` between the builds then is within 1e-5 like every other tensor's
    (measured 3.0e-6, from 1.5e-1), and the kernels are held to the shipped build at 1e-5 in ``verts`` too."""
    name = "structured/grid_t1"
    a = list(RS.args(name))
    assert RS.centres_on_edges(a).all()
    a[20] = a[20] + torch.tensor([RAY_NUDGE, 0.618 * RAY_NUDGE, 0.0])
    share, keep, dev, *rest = _shipped_deviation(name + f", rays moved by {RAY_NUDGE:g}", a)
    assert share <= MAX_EXCLUDED
    assert dev["grad verts"] <= GRAD_TOL, dev
    _kernels_against_shipped(name + f", rays moved by {RAY_NUDGE:g}", keep, dev, *rest)
