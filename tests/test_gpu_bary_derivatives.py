"""Renderer.bary_derivatives / dm2_bary_derivatives_window on the GPU against the contract's restatement
(tests/bary_derivatives_ref.py): bit-equal through _C and through the module (ray tensors and analytic rays), in a window, with
hand-built ids, with an empty window; not differentiable."""
import numpy as np
import pytest
import torch

import bary_derivatives_ref as bref
import rasterize_ref as rref

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

_CASES = {}


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def case(name, L):
    """rasterize_ref.scene(name), the op's own lists for L layers (numpy) and the views' cameras."""
    if (name, L) not in _CASES:
        s = rref.scene(name)
        layers = _C.rasterize_layers_cuda(s["W"], s["H"], _cu(s["verts"]), _cu(s["faces"]), None, _cu(s["verts_ndc"]),
                                          _cu(s["verts_image"]), _cu(s["ray_o"]), _cu(s["ray_d"]), L)[0]
        mv, proj = bref.scene_cameras(name)
        _CASES[(name, L)] = dict(s, layers=layers.cpu().numpy(), mv=mv, proj=proj, cam=bref.camera_block(mv, proj))
    return _CASES[(name, L)]


def _same(got, want, what):
    for g, w, axis in zip(got, want, "xy"):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == np.float32, (what, axis, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), (what, axis, int((_bits(g) != _bits(w)).sum()))


@pytest.mark.parametrize("name,L", [("soup", 3), ("soup", 17), ("lattice", 3)])
def test_bit_equal_to_restatement(name, L):
    c = case(name, L)
    assert (c["layers"] >= 0).sum() > 5000
    got = _C.bary_derivatives_cuda(_cu(c["layers"]), _cu(c["verts"]), _cu(c["faces"]), _cu(c["cam"]))
    want = bref.forward32(c["layers"], c["verts"], c["faces"], c["cam"], c["W"], c["H"])
    _same(got, want, (name, L))
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0
    assert not got[0].cpu().numpy()[c["layers"] < 0].any()


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("name", ["soup", "lattice"])
def test_module_path(name, analytic):
    """Through Renderer (LayeredRenderer inherits the method), the views picked out of order: the restatement fed the camera block
    the module hands the kernel (inv(mv), inv(proj) of the selected views, by torch.inverse, or the rows of ray_cam)."""
    c = case(name, 3)
    B = c["mv"].shape[0]
    idx = [B - 1] + list(range(B - 1))
    cls = dm2.LayeredRenderer if name == "lattice" else dm2.Renderer
    r = cls(_cu(c["mv"]), _cu(c["proj"]), c["W"], c["H"], "cuda", analytic_rays=analytic)
    assert cls.bary_derivatives is dm2.Renderer.bary_derivatives
    if analytic:
        cam = r.ray_cam[idx]
    else:
        cam = torch.cat((torch.inverse(r.mv[idx]).reshape(-1, 16), torch.inverse(r.proj[idx]).reshape(-1, 16)), dim=1)
    rl = c["layers"][idx]
    verts = _cu(c["verts"]).requires_grad_(True)
    got = r.bary_derivatives(idx, _cu(rl), verts, _cu(c["faces"]))
    assert not got[0].requires_grad and not got[1].requires_grad and got[0].grad_fn is None      # constants of the pipeline
    _same(got, bref.forward32(rl, c["verts"], c["faces"], cam.cpu().numpy(), c["W"], c["H"]), (name, analytic))
    # the float64-inverted block differs from torch.inverse's in the last bits only
    near = bref.forward32(rl, c["verts"], c["faces"], c["cam"][idx], c["W"], c["H"])
    assert np.abs(got[0].cpu().numpy() - near[0]).max() <= 1e-3 * np.abs(near[0]).max()


def test_window_is_the_crop_of_the_frame():
    """Origins that are no multiples of 16, one per view: the window's result is the crop of the full frame's, to the bit."""
    c = case("soup", 3)
    r = dm2.Renderer(_cu(c["mv"]), _cu(c["proj"]), c["W"], c["H"], "cuda", analytic_rays=True)
    idx = [0, 1, 2]
    args = (_cu(c["verts"]), _cu(c["faces"]))
    full = r.bary_derivatives(idx, _cu(c["layers"]), *args)
    pm = np.array([[5, 3], [21, 9], [33, 17]], np.int32)
    ph, pw = 41, 57                                                          # (33 + 57 = 90: the window ends at the frame's edge)
    rl = np.stack([c["layers"][b, pm[b, 1]:pm[b, 1] + ph, pm[b, 0]:pm[b, 0] + pw] for b in range(3)])
    win = r.bary_derivatives(idx, _cu(rl), *args, patch_min=_cu(pm))
    for w, f in zip(win, full):
        want = torch.stack([f[b, pm[b, 1]:pm[b, 1] + ph, pm[b, 0]:pm[b, 0] + pw] for b in range(3)])
        assert torch.equal(w, want) and w.abs().max() > 0
    _same(win, bref.forward32(rl, c["verts"], c["faces"], r.ray_cam.cpu().numpy(), c["W"], c["H"], pm), "window")
    with pytest.raises(AssertionError, match="exceed self.width"):
        r.bary_derivatives(idx, _cu(rl), *args, patch_min=_cu(pm + np.array([[1, 0]], np.int32)))
    with pytest.raises(ValueError, match="negative"):
        r.bary_derivatives(idx, _cu(rl), *args, patch_min=_cu(pm * -1))
    with pytest.raises(ValueError, match="patch_min"):
        r.bary_derivatives(idx, _cu(rl), *args, patch_min=_cu(pm[:2]))
    with pytest.raises(ValueError, match="frame"):
        r.bary_derivatives(idx, _cu(rl), *args)


def test_hand_built_ids_and_bad_faces():
    c = case("soup", 3)
    F, P = c["faces"].shape[0], c["verts"].shape[0]
    rng = np.random.RandomState(4)
    rl = rng.randint(-3, F + 3, c["layers"].shape).astype(np.int32)             # any face at any pixel, ids outside [0, F) on both sides
    rl[0, 0, :3, 0] = [-2 ** 31, 2 ** 31 - 1, F]
    faces = c["faces"].copy()
    faces[5, 1] = P                                                          # a vertex outside [0, P)
    faces[6, 0] = -1
    faces[9, 2] = faces[9, 1]                                                # zero area: D.c == 0
    got = _C.bary_derivatives_cuda(_cu(rl), _cu(c["verts"]), _cu(faces), _cu(c["cam"]))
    want = bref.forward32(rl, c["verts"], faces, c["cam"], c["W"], c["H"])
    _same(got, want, "hand-built")
    dead = (rl < 0) | (rl >= F) | np.isin(rl, (5, 6, 9))
    assert dead.sum() > 100 and not got[0].cpu().numpy()[dead].any() and not got[1].cpu().numpy()[dead].any()
    assert (np.abs(want[0][~dead]).max(-1) > 0).mean() > 0.99
    # no faces, no vertices: zeros without a kernel
    for f, v in ((faces[:0], c["verts"]), (faces, c["verts"][:0])):
        z = _C.bary_derivatives_cuda(_cu(rl), _cu(v), _cu(f), _cu(c["cam"]))
        assert not z[0].any() and not z[1].any()


def test_empty_window_and_argument_checks():
    c = case("soup", 3)
    r = dm2.Renderer(_cu(c["mv"]), _cu(c["proj"]), c["W"], c["H"], "cuda")
    lib = _C.load_library()
    launches = []
    real = lib.dm2_bary_derivatives_window
    lib.dm2_bary_derivatives_window = lambda *a: launches.append(1) or real(*a)
    try:
        for shape in ((3, 0, 10, 3), (3, 10, 0, 3), (3, 10, 10, 0)):
            rl = torch.zeros(shape, dtype=torch.int32, device="cuda")
            dx, dy = r.bary_derivatives([0, 1, 2], rl, _cu(c["verts"]), _cu(c["faces"]), patch_min=_cu(np.zeros((3, 2), np.int32)))
            assert tuple(dx.shape) == shape + (3,) == tuple(dy.shape) and dx.dtype == torch.float32
        assert not launches
    finally:
        lib.dm2_bary_derivatives_window = real
    rl, vs, fc, cam = _cu(c["layers"]), _cu(c["verts"]), _cu(c["faces"]), _cu(c["cam"])
    for args, name in (((rl[0], vs, fc, cam), "render_layers"), ((rl.long(), vs, fc, cam), "render_layers"), ((rl, vs[:, :2], fc, cam), "verts"),
                       ((rl, vs.double(), fc, cam), "verts"), ((rl, vs, fc[:, :2], cam), "faces"), ((rl, vs, fc.long(), cam), "faces"),
                       ((rl, vs, fc, cam[:2]), "ray_cam"), ((rl, vs, fc, cam[:, :16]), "ray_cam")):
        with pytest.raises(RuntimeError, match=name):
            _C.bary_derivatives_cuda(*args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.bary_derivatives_cuda(rl.cpu(), vs.cpu(), fc.cpu(), cam.cpu())
    p = _C._ptr
    out = torch.empty(tuple(rl.shape) + (3,), device="cuda")
    B, H, W, L = rl.shape
    assert lib.dm2_bary_derivatives_window(B, H, W, L, vs.shape[0], -1, None, p(rl), p(vs), p(fc), p(cam), p(out), p(out), None) == 1
    assert lib.dm2_bary_derivatives_window(B, H, W, L, vs.shape[0], fc.shape[0], None, p(rl), p(vs), p(fc), None, p(out), p(out), None) == 1
    assert lib.dm2_bary_derivatives_window(B, H, W, L, vs.shape[0], fc.shape[0], None, p(rl), p(vs), p(fc), p(cam), None, p(out), None) == 1
