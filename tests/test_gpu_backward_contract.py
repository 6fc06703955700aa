"""Phase D of the mask-driven backward (dm2_backward_fast.hip) on the edge vectors B2 carries (T = ro - p0, E1, E2 and rd in place
of ray and corners; group 3 runs the reference's Jacobian on them) and with group 1 folded (tests/test_backward_contract_cpu.py
holds the fold to the form it replaces in float64).  Here the kernels: small frames under a perspective camera, so that ray
directions differ per pixel and no cross product degenerates; every clamp code; both settings of DM2_FLAG_CORRECTED_DV; the three
sources of a pair's coverage; with and without the alpha image's gradient; a frame of large faces for the instantiation with runs
inside the rows; a sliver face and a NaN vertex.

Bar: the forward's colour bit-equal to the oracle, all six gradient tensors within GRAD_TOL = 1e-5 relative L-inf of the oracle
with the same non-finite pattern (tests/util.py check_backward)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import accumulate_scenes as A
from util import GRAD_NAMES, GRAD_TOL, capture_forward_args, check_backward, rel_linf, scenes, to_dev, to_numpy_args

from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

# name -> W, H, faces, seed, depth complexity.  "codes": 3 x 3 tiles, the last column and row partial, faces of ~7 px: most pairs
# are edge pixels whose centre lies outside the face.  "large": 4 x 3 tiles under 24 faces of ~2 tiles' area each.
SCENES = {"codes": (40, 36, 110, 71, 4.0), "large": (64, 48, 24, 72, 8.0)}
SOURCES = {"pool": (1.0, 0), "clip": (1.0, _C.DM2_FLAG_NO_PAIR_POOL), "point": (0.0, 0)}
MODES = {"pool": _C.FWD_POOL, "clip": _C.FWD_MASKS, "point": _C.FWD_POINT}


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


@functools.lru_cache(maxsize=None)
def _scene(name, temp):
    W, H, F, seed, dc = SCENES[name]
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + seed, depth_complexity=dc)
    return tuple(capture_forward_args(sc, [0], [[0, 0]], W, H, temp, 20)[0])


@functools.lru_cache(maxsize=None)
def _upstream(name):
    W, H = SCENES[name][:2]
    rng = np.random.default_rng(SCENES[name][3])
    return (rng.standard_normal((1, H, W, 3)).astype(np.float32), rng.standard_normal((1, H, W)).astype(np.float32),
            rng.standard_normal((1, H, W)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _ref_forward(args_key):
    return _orc().render_forward_cuda(*to_numpy_args(args_key))


@functools.lru_cache(maxsize=None)
def _ref_backward(args_key, name, corrected):
    gc, gd, _ = _upstream(name)
    with np.errstate(all="ignore"):
        return _orc().render_backward_cuda(_ref_forward(args_key), gc, gd, corrected_dv=corrected)


def _hip(args, name, fwd_flags, corrected, alpha=False):
    """Forward and backward of the library -> (colour, six gradients) as numpy."""
    gc, gd, gA = _upstream(name)
    dargs = to_dev(list(args))
    with _flags(fwd_flags), _C.alpha_output(alpha):
        out = _C.render_forward_cuda(*dargs)
        mode = _C.last_forward_mode()
    kw = dict(dL_dout_alpha=torch.from_numpy(gA).cuda()) if alpha else {}
    with _flags(fwd_flags | (_C.DM2_FLAG_CORRECTED_DV if corrected else 0)):
        g = _C.render_backward_cuda(out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(), out[7], out[8],
                                    out[9], out[3], out[4], out[5], out[6], **kw)
    torch.cuda.synchronize()
    return out[1].cpu().numpy(), [x.cpu().numpy() for x in g], mode


def live_codes(args, ref):
    """The clamp code (auxiliary.h:292-329) of every pair the oracle's backward visits, from the oracle's own functions: the
    faces a pixel lists with a live overlap that stand in front of its last contributor."""
    orc = _orc()
    na = to_numpy_args(args)
    W, H = na[2], na[3]
    verts, faces, ray_o, ray_d = na[4], na[5], na[19][0], na[20][0]
    gx = (W + 15) // 16
    nc = ref.n_contrib.reshape(H, W)
    codes = []
    for y in range(H):
        for x in range(W):
            r0, r1 = (int(v) for v in ref.binning.ranges[(y // 16) * gx + x // 16])
            live = set(int(f) for f in ref.binning.face_list[r0:r1][:nc[y, x]])
            for f in ref.buf_tri_id[0, y, x, :ref.buf_tri_cnt[0, y, x]]:
                if int(f) in live:
                    ok, tuv, _ = orc.ray_tri(ray_o[y, x], ray_d[y, x], verts[faces[f]])
                    if ok:
                        codes.append(orc.clamp_bary(float(tuv[1]), float(tuv[2]))[0])
    return np.bincount(np.array(codes), minlength=7)


def test_the_codes_scene_hits_every_clamp_code():
    """(from the oracle alone) every code 0 .. 6 on pairs the backward visits: hundreds in each edge region, ten or more at each
    corner; the per-pixel lists did not overflow, so the listed pairs are all of them."""
    args = _scene("codes", 1.0)
    ref = _ref_forward(args)
    assert (ref.buf_tri_cnt < ref.buf_tri_id.shape[-1]).all()
    n = live_codes(args, ref)
    print("\npairs per clamp code:", n.tolist())
    assert len(n) == 7 and (n >= 10).all() and (n[4:] >= 100).all(), n.tolist()
    assert A.route(args, ref) == "wide"


@pytest.mark.parametrize("corrected", [False, True], ids=["as_written", "corrected_dv"])
@pytest.mark.parametrize("source", ["pool", "clip", "point"])
@pytest.mark.parametrize("name", ["codes", "large"])
def test_gradients_on_every_route(name, source, corrected):
    """The three sources of a pair's coverage (POOL, CLIP, POINT) on the frame that takes the instantiation with runs across the
    rows and on the one that takes runs inside the rows (>= 3 list entries a face), under both derivatives of v."""
    temp, flags = SOURCES[source]
    args = _scene(name, temp)
    ref = _ref_forward(args)
    assert A.route(args, ref) == ("row" if name == "large" else "wide")
    color, grads, mode = _hip(args, name, flags, corrected)
    assert mode == MODES[source]
    assert np.array_equal(color.view(np.uint32), ref.color.view(np.uint32))
    want = _ref_backward(args, name, corrected)
    assert np.abs(want["verts"]).max() > 0 and np.isfinite(want["verts"]).all()
    worst = check_backward(dict(grads=grads, ref_grads=want))
    print(f"\n{name} {source} corrected={corrected}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    if corrected:                                          # (the flag is not a no-op on this scene)
        assert rel_linf(_ref_backward(args, name, False)["verts"], want["verts"]) > 1e-3


@pytest.mark.parametrize("corrected", [False, True], ids=["as_written", "corrected_dv"])
@pytest.mark.parametrize("name", ["codes", "large"])
def test_gradients_with_the_alpha_images_gradient(name, corrected):
    """ALPHA: colour, depth and alpha losses together against the sum of two oracle backwards (tests/test_gpu_alpha.py: with
    blue vertex colours 0 and a blue background of -1 the oracle's blue channel is -T_final = alpha - 1)."""
    from test_gpu_alpha import zero_channel
    orc = _orc()
    args = _scene(name, 1.0)
    ref = _ref_forward(args)
    gc, gd, gA = _upstream(name)
    zref = orc.render_forward_cuda(*to_numpy_args(zero_channel(list(args))))
    gcz = np.zeros_like(gc); gcz[..., 2] = gA
    g1 = _ref_backward(args, name, corrected)
    g2 = orc.render_backward_cuda(zref, gcz, np.zeros_like(gd), corrected_dv=corrected)
    want = {n: (g1[n] if n == "verts_color" else (g1[n].astype(np.float64) + g2[n])) for n in GRAD_NAMES}
    color, grads, mode = _hip(args, name, 0, corrected, alpha=True)
    assert mode == _C.FWD_POOL and np.array_equal(color.view(np.uint32), ref.color.view(np.uint32))
    worst = check_backward(dict(grads=grads, ref_grads=want))
    print(f"\n{name} alpha corrected={corrected}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- non-finite gradients stay in the rows of the face that made them -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _front_face(name):
    """The nearest face among those with pairs: no pixel has a face in front of it, so what it does to its pixels' colour and
    depth reaches no other face's dL/dalpha (the replay hands a pair what lies BEHIND it)."""
    args = _scene(name, 1.0)
    ref = _ref_forward(args)
    F = args[5].shape[0]
    listed = np.zeros(F, bool)
    for ids, cnt in zip(ref.buf_tri_id.reshape(-1, ref.buf_tri_id.shape[-1]), ref.buf_tri_cnt.reshape(-1)):
        listed[ids[:cnt]] = True
    depths = np.where(listed, ref.binning.depths[:F], np.inf)
    f = int(np.argmin(depths))
    assert listed.sum() > F // 2 and (depths[np.arange(F) != f] > depths[f]).all()
    return f


def _contained(args, name, corrected, BAD_FACE):
    """The assertions of test_gpu_coverage.py::test_non_finite_gradient_of_a_sliver_face_is_contained and
    test_gpu_backward_accumulate.py::test_nan_vertex_stays_in_its_face on the default route: non-finite rows of dL/dverts are
    the bad face's own at most, as in the oracle; every other row and every other tensor's other faces finite and at the bar."""
    orc = _orc()
    ref = orc.render_forward_cuda(*to_numpy_args(args))
    gc, gd, _ = _upstream(name)
    with np.errstate(all="ignore"):
        want = orc.render_backward_cuda(ref, gc, gd, corrected_dv=corrected)
    own_rows = {3 * BAD_FACE, 3 * BAD_FACE + 1, 3 * BAD_FACE + 2}
    bad_ref = ~np.isfinite(want["verts"]).all(axis=1)
    assert bad_ref.any() and set(np.where(bad_ref)[0]) <= own_rows
    color, grads, mode = _hip(args, name, 0, corrected)
    assert mode == _C.FWD_POOL
    both_nan = np.isnan(color) & np.isnan(ref.color)
    assert np.array_equal(np.isnan(color), np.isnan(ref.color))
    assert np.array_equal(color.view(np.uint32)[~both_nan], ref.color.view(np.uint32)[~both_nan])
    g = dict(zip(GRAD_NAMES, grads))
    bad = ~np.isfinite(g["verts"]).all(axis=1)
    assert set(np.where(bad)[0]) <= own_rows, np.where(bad)[0]
    ok = ~bad_ref & ~bad
    assert rel_linf(g["verts"][ok], want["verts"][ok]) <= GRAD_TOL
    face = np.arange(args[5].shape[0]) == BAD_FACE
    vrow = np.zeros(args[4].shape[0], bool); vrow[list(own_rows)] = True
    for n, x, w in (("verts_color", g["verts_color"][~vrow], want["verts_color"][~vrow]),
                    ("faces_opacity", g["faces_opacity"][~face], want["faces_opacity"][~face]),
                    ("verts_ndc", g["verts_ndc"][:, ~vrow], want["verts_ndc"][:, ~vrow]),
                    ("faces_intense", g["faces_intense"][:, ~face], want["faces_intense"][:, ~face]),
                    ("aa_face_verts", g["aa_face_verts"][:, ~face], want["aa_face_verts"][:, ~face])):
        assert np.isfinite(x).all() and np.isfinite(w).all() and rel_linf(x, w) <= GRAD_TOL, n
    return g, want


@pytest.mark.parametrize("corrected", [False, True], ids=["as_written", "corrected_dv"])
def test_sliver_face_is_contained(corrected):
    """One face whose WORLD triangle is 1e-13 across (image-space tables unchanged): v1 is tiny, 1 / v1^2 overflows, and the
    Jacobian of that face's pairs is Inf or NaN -- in its own lanes and rows only."""
    BAD_FACE = _front_face("codes")
    args = list(_scene("codes", 1.0))
    verts = args[4].clone()
    assert args[4].shape[0] == 3 * args[5].shape[0]                        # (a soup without shared vertices)
    verts[3 * BAD_FACE] = torch.tensor([0.0, 0.0, 0.0]); verts[3 * BAD_FACE + 1] = torch.tensor([1e-13, 0.0, 0.0])
    verts[3 * BAD_FACE + 2] = torch.tensor([0.0, 1e-13, 0.0])
    args[4] = verts
    g, want = _contained(args, "codes", corrected, BAD_FACE)
    for n in GRAD_NAMES[1:]:                                               # (the sliver's own other gradients are finite too)
        assert np.isfinite(g[n]).all() and rel_linf(g[n], want[n]) <= GRAD_TOL, n


@pytest.mark.parametrize("corrected", [False, True], ids=["as_written", "corrected_dv"])
def test_nan_vertex_is_contained(corrected):
    """One NaN world-space corner: the face's pairs carry NaN through B2's edge vectors into every group of phase D."""
    BAD_FACE = _front_face("codes")
    args = list(_scene("codes", 1.0))
    verts = args[4].clone()
    verts[3 * BAD_FACE + 1, 0] = float("nan")
    args[4] = verts
    g, _ = _contained(args, "codes", corrected, BAD_FACE)
    assert not np.isfinite(g["verts"][3 * BAD_FACE:3 * BAD_FACE + 3]).all()
