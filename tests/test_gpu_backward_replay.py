"""The backward's per-pixel replay (phase C of dm2_backward_fast.hip) and the dL/dalpha it leaves to the head of phase D, on
scenes built for it (tests/backward_replay_scenes.py): several records of one pixel in one chunk, state carried across chunks,
alpha == 1 on a last contributor, an opaque only contributor, pixels that end early beside pixels that go on.  Every case first
asserts from the oracle's forward state that its situation is there, then holds every gradient tensor to the oracle at GRAD_TOL,
for every source of a pair's coverage (POOL, CLIP, POINT) and with and without the alpha image's gradient (ALPHA).

ALPHA: the reference is the zero-channel render of tests/test_gpu_alpha.py; on chosen pixels dL/dcolour = 0 and
dL/ddepth = dL/dalpha = 0.5, so that K = bg . g_c + g_d - g_A is exactly 0 there."""
import contextlib

import numpy as np
import pytest
import torch

import backward_replay_scenes as brs
from util import GRAD_NAMES, GRAD_TOL, check_backward, check_forward, rel_linf, run_both, to_dev, to_numpy_args

from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

SOURCES = ["pool", "clip", "point"]


def _orc():
    from oracle import cpu as orc
    return orc


@contextlib.contextmanager
def _flags(f):
    old = _C.set_flags(f)
    try:
        yield
    finally:
        _C.set_flags(old)


def _build(scene, frame, temp):
    if scene == "opaque":
        return brs.opaque_scene(frame, temp)
    if scene.startswith("threshold"):
        return brs.threshold_scene(frame, int(scene[9:]), temp)
    return brs.stack_scene(frame, int(scene[5:]), temp)


def _k_zero_pixels(scene, args, ref, info):
    """(H, W) bool: where the ALPHA cases make K exactly 0 -- on pixels the scene exists for."""
    m = np.zeros((args[3], args[2]), dtype=bool)
    if scene == "opaque":
        fronted, alone, _ = brs.present_opaque(args, ref, info)
        picks = [np.argwhere(fronted)[0], np.argwhere(alone)[0]]
    elif scene.startswith("threshold"):
        picks = [np.argwhere(brs.present_threshold(args, ref, info))[0]]
    else:
        picks = [np.argwhere(brs.present_stack(args, ref, info))[0]]
    for y, x in picks:
        m[y, x] = True
    return m


def _run_alpha(args, ref, kz):
    """Colour, depth and alpha losses together (tests/test_gpu_straightline.py::test_scene_with_alpha_gradient)."""
    from test_gpu_alpha import zero_channel
    orc = _orc()
    H, W = args[3], args[2]
    zref = orc.render_forward_cuda(*to_numpy_args(zero_channel(args)))
    rng = np.random.default_rng(12)
    gc = rng.standard_normal((1, H, W, 3)).astype(np.float32)
    gd = rng.standard_normal((1, H, W)).astype(np.float32)
    gA = rng.standard_normal((1, H, W)).astype(np.float32)
    gc[0][kz] = 0.0; gd[0][kz] = 0.5; gA[0][kz] = 0.5
    bg = np.asarray(brs.BACKGROUND, np.float32)
    K = (((np.float32(0) + bg[0] * gc[..., 0]) + bg[1] * gc[..., 1]) + bg[2] * gc[..., 2]) + gd - gA   # float32, the kernel's order
    assert K.dtype == np.float32 and (K[0][kz] == 0).all() and (K[0][~kz] != 0).all() and (gA != 0).all()
    g1 = orc.render_backward_cuda(ref, gc, gd)
    gcz = np.zeros_like(gc); gcz[..., 2] = gA
    g2 = orc.render_backward_cuda(zref, gcz, np.zeros_like(gd))
    dargs = to_dev(args)
    with _C.alpha_output(True):
        out = _C.render_forward_cuda(*dargs)
    g = _C.render_backward_cuda(out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(), out[7], out[8],
                                out[9], out[3], out[4], out[5], out[6], dL_dout_alpha=torch.from_numpy(gA).cuda())
    assert np.array_equal(out[1].cpu().numpy().view(np.uint32), ref.color.view(np.uint32))
    grads = [x.cpu().numpy() for x in g]
    want = {n: (g1[n] if n == "verts_color" else g1[n].astype(np.float64) + g2[n]) for n in GRAD_NAMES}
    return grads, want


_RUNS = {}


def _run(scene, frame, source, alpha):
    """One forward + backward per (scene, frame, source, alpha), shared by the cases that look at it; every gradient tensor
    held to the oracle here."""
    key = (scene, frame, source, alpha)
    if key in _RUNS:
        return _RUNS[key]
    temp = 0.0 if source == "point" else 1.0
    args, info = _build(scene, frame, temp)
    with _flags(_C.DM2_FLAG_NO_PAIR_POOL if source == "clip" else 0):
        if alpha:
            ref = _orc().render_forward_cuda(*to_numpy_args(args))
            grads, want = _run_alpha(args, ref, _k_zero_pixels(scene, args, ref, info))
        else:
            res = run_both(args, seed=21)
            ref, grads, want = res["ref"], res["grads"], res["ref_grads"]
            check_forward(res, args)
            check_backward(res)
        assert _C.last_forward_mode() == {"pool": _C.FWD_POOL, "clip": _C.FWD_MASKS, "point": _C.FWD_POINT}[source]
    worst = {}
    for name, x in zip(GRAD_NAMES, grads):
        assert x.shape == want[name].shape and np.isfinite(x).all(), name
        worst[name] = rel_linf(x, want[name])
        assert np.abs(want[name]).max() > 0 or (name == "aa_face_verts" and temp == 0.0), name
    print(scene, frame, source, "alpha" if alpha else "plain", worst)
    assert all(v <= GRAD_TOL for v in worst.values()), worst
    _RUNS[key] = (args, info, ref, dict(zip(GRAD_NAMES, grads)), want)
    return _RUNS[key]


def _cases(f):
    for name, values in (("alpha", [False, True]), ("source", SOURCES), ("frame", list(brs.FRAMES))):
        f = pytest.mark.parametrize(name, values, ids=[f"{name}={v}" if name == "alpha" else str(v) for v in values])(f)
    return f


@_cases
def test_several_records_of_a_pixel_in_one_chunk(frame, source, alpha):
    """24 small faces on the same pixels: one chunk holds every pair of the tile, and a pixel owns 24 of its records."""
    args, info, ref, _, _ = _run("stack24", frame, source, alpha)
    assert brs.present_stack(args, ref, info).sum() >= 2


@_cases
def test_state_carried_across_chunks(frame, source, alpha):
    """70 faces: more entries than a chunk has candidates, more pairs than lanes; T and the accumulators live in registers
    from chunk to chunk."""
    args, info, ref, _, _ = _run("stack70", frame, source, alpha)
    brs.present_stack(args, ref, info)
    assert (ref.n_contrib > 30).any()


@_cases
def test_alpha_one_on_a_last_contributor(frame, source, alpha):
    """An opacity-1 face of coverage 1 ends pixels that three faces in front of it blended into, ten faces behind it."""
    args, info, ref, _, _ = _run("opaque", frame, source, alpha)
    fronted, _, _ = brs.present_opaque(args, ref, info)
    assert fronted.any() and (ref.final_T.reshape(fronted.shape)[fronted] == 0).all()


@_cases
def test_first_record_of_a_pixel_whose_final_T_is_zero(frame, source, alpha):
    """The opaque face as a pixel's only contributor: its first replayed record, T_final == 0."""
    args, info, ref, _, _ = _run("opaque", frame, source, alpha)
    _, alone, _ = brs.present_opaque(args, ref, info)
    assert alone.any() and (ref.final_prev_T.reshape(alone.shape)[alone] == 1).all()


@_cases
def test_records_behind_a_last_contributor_stay_out(frame, source, alpha):
    """Pixels that end at the opaque face while their neighbours go on to the tile's last entry: the face that only those
    pixels see gets nothing, exactly."""
    args, info, ref, grads, want = _run("opaque", frame, source, alpha)
    brs.present_guard(args, ref, info)
    h = brs.HIDDEN
    for name, rows in (("faces_opacity", np.s_[h]), ("faces_intense", np.s_[:, h]), ("verts_color", np.s_[3 * h:3 * h + 3]),
                       ("verts", np.s_[3 * h:3 * h + 3]), ("aa_face_verts", np.s_[:, h])):
        assert not np.asarray(want[name])[rows].any() and not grads[name][rows].any(), name
    assert np.abs(grads["faces_opacity"][h + 1:]).min() > 0                     # the faces behind it, seen by the neighbours


@_cases
def test_the_stop_is_strictly_below_T_EPS(frame, source, alpha):
    """Pixels whose transmittance behind two faces is T_EPS to the bit, one ulp below it and one above (brs.threshold_scene):
    the forward's state bit for bit (n_contrib: T < T_EPS, not <=, ends a pixel -- a pixel that stopped one face early keeps
    its colour to 1e-4 and its gradients within GRAD_TOL of nothing, so only the integer state shows it) and every gradient.
    Found by the mutation audit: no scene of the render op reached the equality."""
    for step in brs.THRESHOLD_STEPS:
        args, info, ref, _, _ = _run(f"threshold{step}", frame, source, alpha)
        full = brs.present_threshold(args, ref, info)
        if alpha:                                      # (_run's alpha branch compares colour only: the integer state here)
            dargs = to_dev(args)
            with _C.alpha_output(True):
                out = _C.render_forward_cuda(*dargs)
            check_forward(dict(out=out[:10], ref=ref), args)
        assert full.sum() >= 6
