"""Renderer.rasterize(overlap=True) and Renderer.coverage(inside=...) on the GPU against tests/overlap_ref.py: the five outputs
bit for bit (scenes, L, existence flags, windows, long lists, analytic rays), the backward within GRAD_TOL of the float64
gradients with the clamp codes held fixed (dense and sparse upstream gradients, the table's overflow route), coverage with the
mask, the argument checks, and the acceptance test of the mode: the deferred path on overlap lists reproduces
Renderer.forward's colour, depth and alpha images and their gradients, which it does not on the standard lists."""
import numpy as np
import pytest
import torch

import coverage_ref as cref
import overlap_ref as oref
import tet_scenes as S
import upstream as up
import window_ref as wref
from util import GRAD_TOL, rel_linf, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
LS = (1, 4, 17)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what):
    got = _np(got) if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))


def _rasterize(s, fe, L, win, overlap=True):
    """_C.rasterize_layers_cuda on scene ``s`` over the window (patch_min, pw, ph) with its cut of the rays."""
    fixed = (_cu(s["verts"]), _cu(s["faces"]), _cu(fe), _cu(s["verts_ndc"]), _cu(s["verts_image"]))
    pm, pw, ph = win
    ro, rd = wref.rays(s, pm, pw, ph)
    with _C.window(_cu(pm), s["W"], s["H"]):
        return _C.rasterize_layers_cuda(pw, ph, *fixed, _cu(ro), _cu(rd), L, overlap=overlap)


def _backward(s, layers, win, gb, gt):
    pm, pw, ph = win
    ro, rd = wref.rays(s, pm, pw, ph)
    with _C.window(_cu(pm), s["W"], s["H"]):
        return _np(_C.rasterize_layers_backward_cuda(_cu(layers), _cu(s["verts"]), _cu(s["faces"]), _cu(ro), _cu(rd), _cu(gb), _cu(gt),
                                                     overlap=True))


# ---- forward ---------------------------------------------------------------------------------------------------------------------
FORWARD = [(n, w) for n in oref.SCENES for w in (None, "c", "d", "e")]


@pytest.mark.parametrize("name,win", FORWARD)
def test_forward_bit_equal_to_restatement(name, win):
    """L = 1, 4, 17 (k_rasterize_overlap<1>, <4> and <16> with a second pass); on the full frame and window (c) with and without
    existence flags: ids, counts, clamped barycentrics, t and inside bit-equal to the restatement.  The full frame goes through
    the call without a window as well."""
    s = oref.scene(name)
    w = oref.window_of(name, win)
    for exist in ((False, True) if win in (None, "c") else (False,)):
        x = oref.evaluated(name, win, exist)
        fe = s["fe"] if exist else None
        for L in LS:
            want = oref.select(x, L)
            got = _rasterize(s, fe, L, w)
            assert got[4].dtype == torch.bool
            for k, g in zip(oref.OUTS, got):
                _same(g, want[k], (name, win, L, exist, k))
        if win != "e":
            assert want["cnt"].max() > 1 and ((want["layers"] >= 0) & ~want["inside"]).any()
    if win is None:
        got = _C.rasterize_layers_cuda(s["W"], s["H"], _cu(s["verts"]), _cu(s["faces"]), _cu(fe), _cu(s["verts_ndc"]), _cu(s["verts_image"]),
                                       _cu(s["ray_o"]), _cu(s["ray_d"]), 17, overlap=True)
        for k, g in zip(oref.OUTS, got):
            _same(g, want[k], (name, "no window", k))


def test_long_lists_on_the_crowded_scene():
    """More than 256 candidates in every tile (several LDS chunks) at unaligned window origins, L = 4 and 17."""
    s = oref.scene("crowded")
    x = oref.evaluated("crowded", "crowded", True)
    assert (x["cand"] >= 0).sum(1).min() > 256
    for L in (4, 17):
        want = oref.select(x, L)
        got = _rasterize(s, s["fe"], L, oref.CROWDED_WINDOW)
        for k, g in zip(oref.OUTS, got):
            _same(g, want[k], ("crowded", L, k))
    assert want["cnt"].max() == 17


def test_standard_mode_is_untouched():
    """overlap=False is the call without the keyword: the same 4-tuple, bit for bit."""
    s = oref.scene("soup")
    w = oref.window_of("soup", "c")
    a = _rasterize(s, s["fe"], 4, w, overlap=False)
    pm, pw, ph = w
    ro, rd = wref.rays(s, pm, pw, ph)
    with _C.window(_cu(pm), s["W"], s["H"]):
        b = _C.rasterize_layers_cuda(pw, ph, _cu(s["verts"]), _cu(s["faces"]), _cu(s["fe"]), _cu(s["verts_ndc"]), _cu(s["verts_image"]),
                                     _cu(ro), _cu(rd), 4)
    assert len(a) == len(b) == 4
    for g, h in zip(a, b):
        _same(g, _np(h), "standard")


def _module_scene(analytic):
    """Tet scene "aligned" with a LayeredRenderer that computes its rays, or reads the same rays, as the oracle computes them."""
    from oracle import cpu as orc
    ts, _ = S.case("aligned")
    scd = ts.to("cuda")
    lr = S.renderer(ts, "cuda", analytic_rays=analytic)
    if not analytic:
        ref = S.renderer(ts, "cuda", analytic_rays=True)
        cam = ref.ray_cam.cpu().numpy()
        ro, rd = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), ts.width, ts.height)
        lr.ray_o, lr.ray_d = _cu(ro), _cu(rd)
    return ts, scd, lr


@pytest.mark.parametrize("win", [None, "c"])
def test_analytic_rays_bit_equal_to_the_ray_tensor_path(win):
    """LayeredRenderer.rasterize(overlap=True), forward and backward: the module that computes each pixel's ray gives the bits
    of the module that reads the oracle's analytic rays from tensors."""
    bidx, L = [1, 0], 5
    res = []
    for analytic in (True, False):
        ts, scd, lr = _module_scene(analytic)
        kw = {}
        if win is not None:
            pm, pw, ph = wref.windows(ts.width, ts.height)[win]
            kw = dict(patch_min=_cu(pm), patch_width=pw, patch_height=ph)
        v = scd.verts.clone().requires_grad_(True)
        ras = lr.rasterize(bidx, v, scd.faces, L, faces_existence=scd.faces_existence, overlap=True, **kw)
        assert len(ras) == 5 and ras[4].dtype == torch.bool and not ras[4].requires_grad
        gb = torch.randn(ras[2].shape, generator=torch.Generator().manual_seed(7)).cuda()
        gt = torch.randn(ras[3].shape, generator=torch.Generator().manual_seed(8)).cuda()
        ((ras[2] * gb).sum() + (ras[3] * gt).sum()).backward()
        res.append(([_np(x) for x in ras], _np(v.grad)))
    for k, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        assert np.array_equal(_bits(a), _bits(b)), (win, k)
    assert ((res[0][0][0] >= 0) & ~res[0][0][4]).any() and np.abs(res[0][1]).max() > 0
    assert rel_linf(res[0][1], res[1][1]) <= 2e-6            # (test_gpu_rasterize.py's bar for the same comparison)


# ---- backward --------------------------------------------------------------------------------------------------------------------
def _upstream(shape, seed):
    gen = np.random.default_rng(seed)
    return gen.standard_normal(shape + (3,)).astype(f32), gen.standard_normal(shape).astype(f32)


@pytest.mark.parametrize("name,win,L", [("soup", None, 4), ("soup", "c", 17), ("lattice", None, 4), ("aligned", None, 4), ("degenerate", None, 4)])
def test_backward_within_tolerance_of_float64(name, win, L):
    """dL/dverts for upstream gradients on bary, on t and on both: within GRAD_TOL of the largest entry of ``grads64``; every
    clamp code takes part."""
    s = oref.scene(name)
    w = oref.window_of(name, win)
    pm, pw, ph = w
    sel = oref.select(oref.evaluated(name, win, False), L)
    ro, rd = wref.rays(s, pm, pw, ph)
    codes = oref.slot_codes(s["verts"], s["faces"], sel["layers"], ro, rd)
    assert (np.bincount(codes[codes >= 0], minlength=7) > 0).all(), np.bincount(codes[codes >= 0], minlength=7)
    gb, gt = _upstream(sel["layers"].shape, L)
    for g_b, g_t in ((gb, gt), (gb, None), (None, gt)):
        got = _backward(s, sel["layers"], w, g_b, g_t)
        want = oref.grads64(s["verts"], s["faces"], sel["layers"], ro, rd, g_b, g_t, codes)
        assert np.isfinite(got).all() and np.abs(want).max() > 0
        print(name, win, L, g_b is None, g_t is None, rel_linf(got, want))
        assert rel_linf(got, want) <= GRAD_TOL, (name, win, L, g_b is None, g_t is None, rel_linf(got, want))


@pytest.mark.parametrize("family", up.SLOT_FAMILIES)
def test_backward_under_sparse_upstream(family):
    """tests/upstream.py's slot families on the soup, window (c): the gradient within GRAD_TOL of ``grads64``'s largest entry
    under the masked upstream gradients, and exactly zero at every vertex that no slot with a non-zero upstream gradient names."""
    s = oref.scene("soup")
    w = oref.window_of("soup", "c")
    pm, pw, ph = w
    sel = oref.select(oref.evaluated("soup", "c", False), 4)
    ro, rd = wref.rays(s, pm, pw, ph)
    gb, gt = _upstream(sel["layers"].shape, 11)
    weight = sel["cnt"]
    gbm, kb = up.mask_slots(family, gb, weight)
    gtm, kt = up.mask_slots("one_tile" if family == "one_channel" else family, gt, weight)
    got = _backward(s, sel["layers"], w, gbm, gtm)
    want = oref.grads64(s["verts"], s["faces"], sel["layers"], ro, rd, gbm, gtm)
    live = (sel["layers"] >= 0) & (((gbm != 0).any(-1)) | (gtm != 0))
    touched = np.zeros(s["verts"].shape[0], bool)
    touched[s["faces"][sel["layers"][live]].reshape(-1)] = True
    assert (got[~touched] == 0).all()
    if family == "all_zero":
        assert not live.any() and (got == 0).all()
        return
    assert live.any() and np.abs(want).max() > 0
    print(family, rel_linf(got, want), int(live.sum()))
    assert rel_linf(got, want) <= GRAD_TOL, (family, rel_linf(got, want))


def test_backward_table_overflow_route():
    """k_rasterize_overlap_bwd where the block's table finds no slot: the crowded scene at unaligned window origins, L = 8, lists
    more distinct faces in every window tile than the table holds."""
    s = oref.scene("crowded")
    w = oref.CROWDED_WINDOW
    pm, pw, ph = w
    sel = oref.select(oref.evaluated("crowded", "crowded", False), 8)
    counts = [len(np.unique(t[t >= 0])) for b in range(2) for ty in range(0, ph, 16) for tx in range(0, pw, 16)
              for t in [sel["layers"][b, ty:ty + 16, tx:tx + 16]]]
    assert min(counts) > table_capacity(), (counts, table_capacity())
    got5 = _rasterize(s, None, 8, w)
    _same(got5[0], sel["layers"], "crowded layers")
    ro, rd = wref.rays(s, pm, pw, ph)
    gb, gt = _upstream(sel["layers"].shape, 3)
    for g_b, g_t in ((gb, gt), (None, gt)):
        got = _backward(s, sel["layers"], w, g_b, g_t)
        want = oref.grads64(s["verts"], s["faces"], sel["layers"], ro, rd, g_b, g_t)
        print("overflow", g_b is None, rel_linf(got, want))
        assert rel_linf(got, want) <= GRAD_TOL, rel_linf(got, want)


# ---- coverage with the mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 3])
@pytest.mark.parametrize("win", [None, "c"])
def test_coverage_with_inside_bit_equal_and_gradients(L, win):
    """coverage(inside=...) at temperatures 1, 0.5 and 0 on both id paths (L % 4 == 0: k_coverage<4, true>; L = 3: <1, true>),
    bool and integer masks: bit-equal to the restatement; the gradient, whose form the mask does not change, within GRAD_TOL of
    ``coverage_ref.grad_image64``."""
    s = oref.scene("soup")
    pm, pw, ph = oref.window_of("soup", win)
    sel = oref.select(oref.evaluated("soup", win, False), L)
    rl, ins = sel["layers"], sel["inside"]
    frame_rl, frame_in = wref.embed(rl, pm, s["W"], s["H"], -1), wref.embed(ins, pm, s["W"], s["H"], False)
    g = cref.upstream(rl.shape, 17 + L)
    for temp in cref.TEMPERATURES:
        cov_f, info = oref.coverage32(frame_rl, frame_in, s["verts_image"], s["faces"], temp)
        want = wref.cut(cov_f, pm, pw, ph)
        for mask in (_cu(ins), _cu(ins.astype(np.int32) * 5), _cu(ins.astype(np.uint8))):
            with _C.window(_cu(pm) if win else None, s["W"], s["H"]):
                got = _C.coverage_cuda(_cu(rl), _cu(s["verts_image"]), _cu(s["faces"]), temp, inside=mask)
            _same(got, want, (L, win, temp, mask.dtype))
        off = (rl >= 0) & ~ins
        assert off.any() and ((want[off] > 0).all() if temp > 0 else (want[off] == 0).all())
        with _C.window(_cu(pm) if win else None, s["W"], s["H"]):
            plain = _np(_C.coverage_cuda(_cu(rl), _cu(s["verts_image"]), _cu(s["faces"]), temp))
        assert np.array_equal(_bits(plain[~off]), _bits(want[~off]))
        # (1 - temperature) + area * temperature against area * temperature: one value at temperature 1, else not
        assert np.array_equal(_bits(plain[off]), _bits(want[off])) if temp == 1.0 else (plain[off] != want[off]).all()
        if temp > 0:
            with _C.window(_cu(pm) if win else None, s["W"], s["H"]):
                gi = _np(_C.coverage_backward_cuda(_cu(rl), _cu(s["verts_image"]), _cu(s["faces"]), temp, _cu(g)))
            ref = cref.grad_image64(frame_rl, s["verts_image"], s["faces"], temp, wref.embed(g, pm, s["W"], s["H"], 0), info)
            assert rel_linf(gi, ref) <= GRAD_TOL, (L, win, temp, rel_linf(gi, ref))


# ---- the equivalence with Renderer.forward ---------------------------------------------------------------------------------------
def _stair_tensors():
    s = oref.scene("staircase")
    t = {k: _cu(s[k]) for k in ("verts", "faces", "verts_color", "faces_opacity", "faces_intense", "background")}
    r = dm2.Renderer(_cu(s["mv"]), _cu(s["proj"]), s["W"], s["H"], "cuda")
    return s, t, r


def _leaves(t):
    return [t[k].clone().requires_grad_(True) for k in ("verts", "verts_color", "faces_opacity")]


def _deferred(r, t, leaves, win, temp, overlap):
    """rasterize -> interpolate -> coverage -> composite: colour, depth and alpha as Renderer.forward returns them."""
    verts, vcol, opac = leaves
    bidx = [0, 1]
    kw = {} if win is None else dict(patch_min=_cu(win[0]), patch_width=win[1], patch_height=win[2])
    ras = r.rasterize(bidx, verts, t["faces"], oref.STAIR_L, overlap=overlap, **kw)
    layers, bary = ras[0], ras[2]
    inside = ras[4] if overlap else None
    ids = layers.clamp(min=0).long()
    B = layers.shape[0]
    ndc, _ = r.compute_verts_ndc_image(verts, r.mv[bidx], r.proj[bidx])
    col = r.interpolate(layers, bary, vcol, t["faces"]) * t["faces_intense"][torch.arange(B, device="cuda").view(B, 1, 1, 1), ids][..., None]
    dep = r.interpolate(layers, bary, ndc[..., 2:3].contiguous(), t["faces"])
    cov = r.coverage(bidx, layers, verts, t["faces"], temperature=temp, patch_min=None if win is None else _cu(win[0]), inside=inside)
    out, acc = r.composite(torch.cat([col, dep], -1), opac[ids] * cov, layers, torch.cat([t["background"], torch.ones(1, device="cuda")]))
    return out[..., :3], 1.0 - (out[..., 3] + 1.0) / 2.0, acc, ras


def _forward(r, t, leaves, win, temp):
    verts, vcol, opac = leaves
    B = 2
    pm = torch.zeros((B, 2), dtype=torch.int32, device="cuda") if win is None else _cu(win[0])
    pw, ph = (r.width, r.height) if win is None else (win[1], win[2])
    return r.forward([0, 1], pm, pw, ph, verts, t["faces"], vcol, opac, t["faces_intense"], t["background"], aa_temperature=temp,
                     return_alpha=True)


@pytest.mark.parametrize("temp", [1.0, 0.5])
@pytest.mark.parametrize("win", [None, "patch"])
def test_deferred_path_reproduces_forward(win, temp):
    """The acceptance test.  On the staircase scene (tests/test_overlap_cpu.py shows that it lists nothing ambiguous and that
    the float32 restatements of the two paths lie 1.2e-7 of the maximum apart) the deferred path on overlap lists gives
    Renderer.forward's colour, depth and alpha within 1e-5 of each tensor's maximum, and so the gradients of one loss on all
    three w.r.t. verts, verts_color and faces_opacity (forward's backward with the corrected dv, the derivative the deferred
    path computes).  Control: on the standard lists alpha differs, at silhouette pixels only, and the lists differ there."""
    s, t, r = _stair_tensors()
    w = None if win is None else oref.STAIR_PATCH
    gen = torch.Generator().manual_seed(5)
    old = _C.set_flags(_C.DM2_FLAG_CORRECTED_DV)
    try:
        la = _leaves(t)
        fc, fd, fa = _forward(r, t, la, w, temp)
        gc, gd, ga = (torch.randn(x.shape, generator=gen).cuda() for x in (fc, fd, fa))
        ((fc * gc).sum() + (fd * gd).sum() + (fa * ga).sum()).backward()
    finally:
        _C.set_flags(old)
    lb = _leaves(t)
    dc, dd, da, ras = _deferred(r, t, lb, w, temp, True)
    assert (ras[0][..., -1] == -1).all()                                         # nothing truncated
    ((dc * gc).sum() + (dd * gd).sum() + (da * ga).sum()).backward()
    for k, a, b in (("color", dc, fc), ("depth", dd, fd), ("alpha", da, fa)):
        print(f"staircase win={win} temp={temp} {k}: {rel_linf(_np(a), _np(b)):.3g}")
        assert rel_linf(_np(a), _np(b)) <= GRAD_TOL, (k, rel_linf(_np(a), _np(b)))
    for k, a, b in zip(("verts", "verts_color", "faces_opacity"), lb, la):
        assert np.abs(_np(b.grad)).max() > 0
        print(f"staircase win={win} temp={temp} d{k}: {rel_linf(_np(a.grad), _np(b.grad)):.3g}")
        assert rel_linf(_np(a.grad), _np(b.grad)) <= GRAD_TOL, (k, rel_linf(_np(a.grad), _np(b.grad)))
    # control: the standard lists
    with torch.no_grad():
        _, _, ca, std = _deferred(r, t, _leaves(t), w, temp, False)
    sil = _np(((ras[0] >= 0) & ~ras[4]).any(-1))
    diff = np.abs(_np(ca).astype(np.float64) - _np(fa)) > GRAD_TOL * float(fa.detach().abs().max())
    assert diff.any() and not (diff & ~sil).any() and rel_linf(_np(ca), _np(fa)) > 1e-3
    assert (_np(std[1]) < _np(ras[1]))[sil].all() and (_np(std[1]) == _np(ras[1]))[~sil].all()


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_arguments():
    s, t, r = _stair_tensors()
    with pytest.raises(ValueError):
        r.rasterize([0, 1], t["verts"], t["faces"], 4, patch_min=_cu(oref.STAIR_PATCH[0]), overlap=True)
    empty = r.rasterize([0, 1], t["verts"], t["faces"], 4, patch_min=_cu(oref.STAIR_PATCH[0]), patch_width=0, patch_height=7, overlap=True)
    assert len(empty) == 5 and all(x.numel() == 0 for x in empty) and empty[4].dtype == torch.bool and empty[4].shape == (2, 7, 0, 4)
    ras = r.rasterize([0, 1], t["verts"], t["faces"], 4, overlap=True)
    with pytest.raises(ValueError):
        r.coverage([0, 1], ras[0], t["verts"], t["faces"], inside=ras[4][..., :3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.coverage_cuda(ras[0], r.compute_verts_ndc_image(t["verts"], r.mv, r.proj)[1], t["faces"], 1.0, inside=ras[4].cpu())
    rc = dm2.Renderer(torch.from_numpy(s["mv"]), torch.from_numpy(s["proj"]), s["W"], s["H"], "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        rc.rasterize([0, 1], t["verts"].cpu(), t["faces"].cpu(), 4, overlap=True)
    assert "RasterizeOverlapFunction" in dm2.__all__


def test_c_abi_refuses_overlap_without_inside():
    """The C ABI refuses what the shim would never send: dm2_rasterize_run in overlap mode with L = 1 and no ``inside``, one
    view of 8 x 8 pixels and one face -> 1 with a message that names ``inside``, before anything is launched (the scratch
    pointers are NULL: a launch would not get that far either)."""
    import ctypes
    dev = "cuda"
    verts = torch.tensor([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.0, 0.5, 0.0]], device=dev)
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    ndc, img = torch.zeros((1, 3, 3), device=dev), torch.zeros((1, 3, 2), device=dev)
    ro, rd = torch.zeros((1, 8, 8, 3), device=dev), torch.ones((1, 8, 8, 3), device=dev)
    keep = []
    d, _ = _C._rasterize_desc(8, 8, 1, verts, faces, ro, rd, 1, keep, verts_ndc=ndc, verts_image=img)
    layers = torch.empty((1, 8, 8, 1), dtype=torch.int32, device=dev)
    cnt = torch.empty((1, 8, 8), dtype=torch.int32, device=dev)
    bary, t = torch.empty((1, 8, 8, 1, 3), device=dev), torch.empty((1, 8, 8, 1), device=dev)
    lib, p = _C.load_library(), _C._ptr
    rc = lib.dm2_rasterize_run(ctypes.byref(d), None, 0, 0, None, 0, None, 0, None, 0, p(layers), p(cnt), p(bary), p(t), 1, None, None)
    assert rc == 1 and b"inside" in lib.dm2_last_error()
