"""Renderer.coverage / dm2_coverage on the GPU against the contract's restatement (tests/coverage_ref.py): the forward bit-equal to
coverage32 on every case (three temperatures, the vector and the scalar id path, NaN-filled outputs), dL/dverts_image within
GRAD_TOL of grad_image64 (the face table's overflow route included), exact zeros where nothing flows, no launch where nothing
can flow, non-finite data nobody lists, the module path rasterize -> coverage -> composite down to verts.grad on both host preps,
camera gradients, a side stream, argument checks and one full-size call."""
import ctypes

import numpy as np
import pytest
import torch

import composite_ref
import coverage_ref as ref
import rasterize_ref as rref
from util import GRAD_TOL, rel_linf, scenes, spy_library

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
MODULE_TOL = 1e-3       # two fp32 routes to one quantity (test_gpu_composite.py, test_gpu_prep.py)
CASES = [f"{n}-L{L}" for n, L in ref.SCENE_CASES] + [f"{n}-{k}" for n, k in ref.FIXTURE_CASES] + ["overflow"]


def _case(label):
    return dict(ref.all_cases())[label]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shifted(a):
    """``a`` on the GPU as a contiguous view that starts 4 bytes into its storage: no 16-byte alignment, the scalar id path."""
    t = _cu(a)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.numel() == 0 or (v.data_ptr() % 16 == 4 and v.is_contiguous())
    return v


def _raw_forward(c, temperature, put=_cu):
    """dm2_coverage through the C entry point into a NaN-filled output -> cov as numpy."""
    lib = _C.load_library()
    rl, vi, fc = put(c["render_layers"]), _cu(c["verts_image"]), _cu(c["faces"])
    B, H, W, L = rl.shape
    out = torch.full((B, H, W, L), float("nan"), device="cuda")
    p = _C._ptr
    rc = lib.dm2_coverage(B, H, W, L, vi.shape[1], fc.shape[0], temperature, None, p(rl), None, p(vi), p(fc), p(out),
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dm2_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("label", CASES)
def test_forward_bit_equal_to_restatement(label):
    c = _case(label)
    L = c["render_layers"].shape[-1]
    for t in ref.TEMPERATURES:
        want = c["info"][t]["cov"]
        got = _raw_forward(c, t)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(_bits(got), _bits(want)), (label, t, int((_bits(got) != _bits(want)).sum()))
        got = _raw_forward(c, t, put=_shifted)                              # (L % 4 == 0: the scalar path instead of the vector one)
        assert np.array_equal(_bits(got), _bits(want)), (label, t, "unaligned", L)
        shim = _C.coverage_cuda(_cu(c["render_layers"]), _cu(c["verts_image"]), _cu(c["faces"]), t).cpu().numpy()
        assert np.array_equal(_bits(shim), _bits(want)), (label, t, "shim")


def _backward(c, temperature, g, put=_cu):
    d = _C.coverage_backward_cuda(put(c["render_layers"]), _cu(c["verts_image"]), _cu(c["faces"]), temperature, _cu(g))
    return None if d is None else d.cpu().numpy()


@pytest.mark.parametrize("label", CASES)
def test_backward_against_float64(label):
    c = _case(label)
    for t in (1.0, 0.5):
        want = ref.grad_image64(c["render_layers"], c["verts_image"], c["faces"], t, c["g"], c["info"][t])
        for put in (_cu, _shifted):
            got = _backward(c, t, c["g"], put)
            assert got.shape == want.shape and np.isfinite(got).all()
            assert not got[want == 0].any(), (label, t)                     # exactly zero where the reference is zero
            if want.any():
                e = rel_linf(got, want)
                print(label, t, put.__name__, e)
                assert e <= GRAD_TOL, (label, t, e)
            else:
                assert label.startswith("no_faces")
        assert not _backward(c, t, np.zeros_like(c["g"])).any()            # a zero upstream gradient: exactly zero
    assert _backward(c, 0.0, c["g"]) is None


def test_no_launch_where_nothing_flows():
    """Temperature 0, cov left out of the loss, verts_image not requiring grad: the backward entry point is not entered; and it is,
    once, otherwise."""
    c = _case("overflow")
    calls = []
    real = _C.load_library().dm2_coverage_backward
    with spy_library(dm2_coverage_backward=lambda *a: calls.append(1) or real(*a)):
        rl, fc = _cu(c["render_layers"]), _cu(c["faces"])
        for t, use in ((0.0, True), (1.0, False)):
            vi = _cu(c["verts_image"]).requires_grad_(True)
            cov = dm2.CoverageFunction.apply(rl, vi, fc, t)
            assert cov.requires_grad
            ((cov * _cu(c["g"])).sum() if use else (vi.sum() + 0 * cov.detach().sum())).backward()
            assert not calls
            assert vi.grad is None if use else bool((vi.grad == 1).all())
        cov = dm2.CoverageFunction.apply(rl, _cu(c["verts_image"]), fc, 1.0)
        assert cov.grad_fn is None and not calls
        vi = _cu(c["verts_image"]).requires_grad_(True)
        (dm2.CoverageFunction.apply(rl, vi, fc, 1.0) * _cu(c["g"])).sum().backward()
        assert len(calls) == 1
        want = ref.grad_image64(c["render_layers"], c["verts_image"], c["faces"], 1.0, c["g"], c["info"][1.0])
        assert rel_linf(vi.grad.cpu().numpy(), want) <= GRAD_TOL
        # the C entry point itself launches nothing at temperature 0 or without an upstream gradient: the NaNs stay
        d = torch.full((1, c["verts_image"].shape[1], 2), float("nan"), device="cuda")
        p = _C._ptr
        B, H, W, L = c["render_layers"].shape
        n = (B, H, W, L, c["verts_image"].shape[1], c["faces"].shape[0])
        assert real(*n, 0.0, None, p(rl), p(vi), p(fc), p(_cu(c["g"])), p(d), None) == 0
        assert real(*n, 1.0, None, p(rl), p(vi), p(fc), None, p(d), None) == 0
        torch.cuda.synchronize()
        assert torch.isnan(d).all()


def test_nonfinite_vertices_nobody_lists():
    """NaN and inf in the verts_image rows that belong only to faces no slot lists: the same bits forward, the same gradient."""
    c = _case("lattice-L3")
    rl, fc, vi = c["render_layers"], c["faces"], c["verts_image"].copy()
    B = vi.shape[0]
    planted = 0
    for b in range(B):
        listed = np.zeros(fc.shape[0], bool)
        ids = rl[b][(rl[b] >= 0)]
        listed[ids] = True
        used = np.zeros(vi.shape[1], bool)
        used[fc[listed].reshape(-1)] = True
        free = np.nonzero(~used)[0]
        vi[b, free[::2]] = np.nan
        vi[b, free[1::2]] = np.inf
        planted += len(free)
    assert planted > 20
    d = dict(c, verts_image=vi)
    for t in (1.0, 0.5):
        assert np.array_equal(_bits(_raw_forward(d, t)), _bits(c["info"][t]["cov"]))
        got = _backward(d, t, c["g"])
        want = ref.grad_image64(rl, c["verts_image"], fc, t, c["g"], c["info"][t])
        assert np.isfinite(got).all() and not got[want == 0].any() and rel_linf(got, want) <= GRAD_TOL


# ---- the module path -----------------------------------------------------------------------------------------------------------
def _lattice(fused, **kw):
    """rasterize_ref.scene("lattice") as a scene on the GPU (the same generator call) -> (renderer, view indices, scene)."""
    ts = scenes.tet_lattice(72, 56, 4, seed=scenes.SEED_BASE + 81, num_cams=2).to("cuda")
    s = rref.scene("lattice")
    assert np.array_equal(ts.verts.cpu().numpy(), s["verts"]) and np.array_equal(ts.faces.cpu().numpy(), s["faces"])
    return dm2.LayeredRenderer(ts.mv, ts.proj, 72, 56, "cuda", fused_prep=fused, **kw), [1, 0], ts


def _image_of(r, bidx, verts, faces):
    """verts_image as the module's own projection computes it."""
    mv, proj = r.mv[bidx], r.proj[bidx]
    with torch.no_grad():
        if r.fused_prep:
            from dmesh2_renderer_amd import prep
            return prep.project(verts, faces.int(), mv, proj, r.width, r.height)[1]
        return r.compute_verts_ndc_image(verts, mv, proj)[1]


@pytest.mark.parametrize("fused", [True, False], ids=["fused_prep", "torch_prep"])
def test_module_path_to_verts(fused):
    """rasterize -> interpolate(colour) -> coverage -> composite with alpha = faces_opacity[ids] * cov, temperature 0.75, a loss over
    out and acc.  cov bit-equal to coverage32 at the module's own verts_image; verts.grad against the CPU chain composite_ref.grads64
    -> grad_image64 -> the oracle's prepare_faces_backward(g_image=...), plus rasterize's part (rasterize_ref.grads64 of the
    barycentrics' gradient) at MODULE_TOL; with loss = acc.sum() verts.grad is non-zero with coverage and exactly zero without."""
    from oracle import cpu as orc
    r, bidx, ts = _lattice(fused)
    assert type(r).coverage is dm2.Renderer.coverage                       # inherited
    L, T, F = 3, 0.75, ts.faces.shape[0]
    gen = torch.Generator().manual_seed(31)
    color = torch.rand((ts.verts.shape[0], 3), generator=gen).cuda()
    op = (torch.rand(F, generator=gen) * 0.85 + 0.05).cuda()
    bg = torch.tensor([0.2, 0.5, 0.9]).cuda()
    verts = ts.verts.clone().requires_grad_(True)
    layers, cnt, bary, t = r.rasterize(bidx, verts, ts.faces, L)
    bary.retain_grad()
    values = r.interpolate(layers, bary, color, ts.faces)
    cov = r.coverage(bidx, layers, verts, ts.faces, temperature=T)
    alpha = op[layers.clamp(min=0).long()] * cov
    alpha.retain_grad()
    out, acc = r.composite(values, alpha, layers, bg)
    wo, wa = torch.randn(out.shape, generator=gen).cuda(), torch.randn(acc.shape, generator=gen).cuda()
    ((out * wo).sum() + (acc * wa).sum()).backward()
    # the CPU chain, from the module's own projection and lists
    rl, vi = layers.cpu().numpy(), _image_of(r, bidx, ts.verts, ts.faces).cpu().numpy()
    fc, vn = ts.faces.cpu().numpy(), values.detach().cpu().numpy()
    info = ref.coverage32(rl, vi, fc, T)
    assert info["partial"].sum() > 3000 and info["full"].sum() > 3000
    assert np.array_equal(_bits(cov.detach().cpu().numpy()), _bits(info["cov"]))
    opn = op.cpu().numpy()[np.where(rl >= 0, rl, 0)]
    an = (opn * info["cov"]).astype(f32)
    assert np.array_equal(_bits(alpha.detach().cpu().numpy()), _bits(an))
    _, _, n = composite_ref.forward32(vn, an, rl, bg.cpu().numpy())
    _, da = composite_ref.grads64(vn, an, rl, bg.cpu().numpy(), n, wo.cpu().numpy(), wa.cpu().numpy())
    assert rel_linf(alpha.grad.cpu().numpy(), da) <= GRAD_TOL
    gi = ref.grad_image64(rl, vi, fc, T, da * opn, info)
    mv, proj = ts.mv[bidx].cpu().numpy(), ts.proj[bidx].cpu().numpy()
    s = rref.scene("lattice")
    want_cov = orc.prepare_faces_backward(s["verts"], fc, mv, proj, 72, 56, g_image=gi, dtype=np.float64)
    ro, rd = r.ray_o[bidx].cpu().numpy(), r.ray_d[bidx].cpu().numpy()             # (the module's own rays)
    want_ras = rref.grads64(s["verts"], fc, rl, ro, rd, bary.grad.cpu().numpy(), None)
    want = want_cov + want_ras
    e = rel_linf(verts.grad.cpu().numpy(), want)
    print("verts.grad", e, "coverage's share", float(np.abs(want_cov).max()), "rasterize's", float(np.abs(want_ras).max()))
    assert np.abs(want_cov).max() > 0.1 * np.abs(want).max() and e <= MODULE_TOL
    # a silhouette loss: acc alone
    for with_cov in (True, False):
        v2 = ts.verts.clone().requires_grad_(True)
        layers2, _, bary2, _ = r.rasterize(bidx, v2, ts.faces, L)
        a2 = op[layers2.clamp(min=0).long()] * (r.coverage(bidx, layers2, v2, ts.faces, temperature=T) if with_cov else 1.0)
        acc2 = r.composite(r.interpolate(layers2, bary2, color, ts.faces), a2, layers2, bg)[1]
        acc2.sum().backward()
        if with_cov:
            assert torch.isfinite(v2.grad).all() and float(v2.grad.abs().max()) > 0
        else:
            assert v2.grad is None or not v2.grad.any()


@pytest.mark.parametrize("fused", [True, False], ids=["fused_prep", "torch_prep"])
def test_camera_gradients(fused):
    ts = scenes.tet_lattice(72, 56, 4, seed=scenes.SEED_BASE + 81, num_cams=2).to("cuda")
    mv, proj = ts.mv.clone().requires_grad_(True), ts.proj.clone().requires_grad_(True)
    r = dm2.Renderer(mv, proj, 72, 56, "cuda", fused_prep=fused)
    with torch.no_grad():
        layers = r.rasterize([1, 0], ts.verts, ts.faces, 3)[0]
    cov = r.coverage([1, 0], layers, ts.verts, ts.faces)
    w = torch.randn(cov.shape, generator=torch.Generator().manual_seed(3)).cuda()
    (cov * w).sum().backward()
    for g in (mv.grad, proj.grad):
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


# ---- a side stream -------------------------------------------------------------------------------------------------------------
class _Delay:
    """About 30 ms of spinning enqueued on ``stream``; ``check`` asserts from events that it took 10 ms or more (without it the
    test would prove nothing)."""
    _rate = []

    def __init__(self, stream, ms=30.0):
        if not self._rate:
            torch.cuda._sleep(1_000_000)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); torch.cuda._sleep(4_000_000); e1.record()
            e1.synchronize()
            self._rate.append(4_000_000 / max(e0.elapsed_time(e1), 1e-3))
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.e0.record(); torch.cuda._sleep(int(ms * self._rate[0])); self.e1.record()

    def check(self):
        self.e1.synchronize()
        t = self.e0.elapsed_time(self.e1)
        assert t >= 10.0, f"the delay took {t} ms: the GPU was not kept busy and the test proves nothing"


@pytest.mark.parametrize("busy", ["side", "default"])
def test_side_stream(busy):
    """The inputs arrive on a side stream only (asynchronous copies from pinned memory into tensors that hold another, valid
    case), behind a delay on that stream or with the default stream kept busy; forward and backward run there and nothing but
    that stream is waited for.  A launch that went elsewhere would read the other case, or results that are not there yet."""
    c = _case("overflow")
    keys = ("render_layers", "verts_image", "faces", "g")
    host = {k: torch.from_numpy(np.ascontiguousarray(c[k])).pin_memory() for k in keys}
    n = c["faces"].shape[0]
    poison = dict(render_layers=(n - 1 - c["render_layers"]).astype(np.int32), verts_image=c["verts_image"][:, ::-1].copy(),
                  faces=c["faces"][::-1].copy(), g=-c["g"])
    want = ref.grad_image64(c["render_layers"], c["verts_image"], c["faces"], 0.5, c["g"], c["info"][0.5])
    for side in (torch.cuda.Stream(), torch.cuda.Stream()):
        dev = {k: _cu(poison[k]) for k in keys}
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            d1 = _Delay(side if busy == "side" else torch.cuda.default_stream())
            for k in keys:
                dev[k].copy_(host[k], non_blocking=True)
            vi = dev["verts_image"].requires_grad_(True)
            cov = dm2.CoverageFunction.apply(dev["render_layers"], vi, dev["faces"], 0.5)
            (cov * dev["g"]).sum().backward()
            side.synchronize()
            got = [x.detach().cpu().numpy() for x in (cov, vi.grad)]
        assert np.array_equal(_bits(got[0]), _bits(c["info"][0.5]["cov"]))
        assert rel_linf(got[1], want) <= GRAD_TOL
        d1.check()
    torch.cuda.synchronize()


def test_argument_checks():
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32, device="cuda")
    vi = torch.zeros((2, 7, 2), device="cuda")
    fc = torch.zeros((6, 3), dtype=torch.int32, device="cuda")
    cov = _C.coverage_cuda(rl, vi, fc, 1.0)
    assert tuple(cov.shape) == (2, 4, 5, 3) and cov.dtype == torch.float32
    for args, name in (((rl[0], vi, fc, 1.0), "render_layers"), ((rl.long(), vi, fc, 1.0), "render_layers"),
                       ((rl.float(), vi, fc, 1.0), "render_layers"), ((rl, vi[:1], fc, 1.0), "verts_image"),
                       ((rl, vi[..., :1], fc, 1.0), "verts_image"), ((rl, vi.double(), fc, 1.0), "verts_image"),
                       ((rl, vi[0], fc, 1.0), "verts_image"), ((rl, vi, fc[:, :2], 1.0), "faces"), ((rl, vi, fc.long(), 1.0), "faces"),
                       ((rl, vi, fc.reshape(-1), 1.0), "faces")):
        with pytest.raises(RuntimeError, match=name):
            _C.coverage_cuda(*args)
    with pytest.raises(RuntimeError, match="grad_cov"):
        _C.coverage_backward_cuda(rl, vi, fc, 1.0, cov[..., :2])
    with pytest.raises(RuntimeError, match="grad_cov"):
        _C.coverage_backward_cuda(rl, vi, fc, 1.0, cov.double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.coverage_cuda(rl.cpu(), vi.cpu(), fc.cpu(), 1.0)
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    verts = torch.zeros((7, 3), device="cuda")
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            _C.coverage_cuda(rl, vi, fc, bad)
        with pytest.raises(ValueError, match="temperature"):
            _C.coverage_backward_cuda(rl, vi, fc, bad, cov)
        with pytest.raises(ValueError, match="temperature"):
            r.coverage([0], rl[:1, :, :, :], verts, fc, temperature=bad)
    # empty sizes: no launch, the shapes of the contract
    assert tuple(_C.coverage_cuda(rl[..., :0], vi, fc, 1.0).shape) == (2, 4, 5, 0)
    assert not _C.coverage_cuda(rl, vi, fc[:0], 1.0).any() and not _C.coverage_cuda(rl, vi[:, :0], fc, 1.0).any()
    assert not _C.coverage_backward_cuda(rl, vi, fc[:0], 1.0, cov).any()
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    p = _C._ptr
    assert lib.dm2_coverage(2, 4, 5, 3, 7, 6, 1.0, None, p(rl), None, p(vi), p(fc), p(cov), None) == 0
    assert lib.dm2_coverage(2, 4, 5, 3, 7, 6, 1.5, None, p(rl), None, p(vi), p(fc), p(cov), None) == 1
    assert lib.dm2_coverage(2, 4, 5, 3, 7, 6, float("nan"), None, p(rl), None, p(vi), p(fc), p(cov), None) == 1
    assert lib.dm2_coverage(2, 4, 5, 3, -1, 6, 1.0, None, p(rl), None, p(vi), p(fc), p(cov), None) == 1
    assert lib.dm2_coverage(2, 4, 5, 3, 7, 6, 1.0, None, None, None, p(vi), p(fc), p(cov), None) == 1
    assert lib.dm2_coverage(2, 4, 5, 3, 7, 6, 1.0, None, p(rl), None, p(vi), None, p(cov), None) == 1
    assert lib.dm2_coverage(2, 4, 5, 3, 7, 6, 1.0, None, p(rl), None, p(vi), p(fc), None, None) == 1
    assert lib.dm2_coverage_backward(2, 4, 5, 3, 7, 6, -1.0, None, p(rl), p(vi), p(fc), p(cov), p(vi), None) == 1
    assert lib.dm2_coverage_backward(2, 4, 5, 3, 7, 6, 1.0, None, None, p(vi), p(fc), p(cov), p(vi), None) == 1
    torch.cuda.synchronize()


def test_full_size():
    """1920 x 1080, L = 4, the 1 M-face soup (SURVEY.md 8(d) cfg 4) on rasterize's lists: finite and within [0, 1], forward and
    backward."""
    sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to("cuda")
    r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, "cuda")
    with torch.no_grad():
        layers = r.rasterize([0], sc.verts, sc.faces, 4)[0]
    verts = sc.verts.clone().requires_grad_(True)
    cov = r.coverage([0], layers, verts, sc.faces, temperature=1.0)
    c = cov.detach()
    assert tuple(c.shape) == (1, 1080, 1920, 4)
    assert bool(torch.isfinite(c).all()) and float(c.min()) >= 0.0 and float(c.max()) <= 1.0
    assert not c[layers < 0].any() and float((c > 0).float().mean()) > 0.2
    assert int(((c > 0) & (c < 1)).sum()) > 100_000
    cov.sum().backward()
    assert bool(torch.isfinite(verts.grad).all()) and float(verts.grad.abs().max()) > 0
