"""Renderer.composite / dm2_composite on the GPU against the contract's restatement (tests/composite_ref.py): the forward
bit-equal to forward32 (out, acc, final_T, n_contrib; vector and scalar paths), the gradients within GRAD_TOL of grads64 for
every combination of upstream and requested gradients, zeros and full coverage of the outputs, non-finite data in slots that
take no part, the face table's overflow route, the module path from rasterize to verts.grad, LayeredRenderer.render as a second
reference, a side stream, argument checks and one full-size case."""
import ctypes

import numpy as np
import pytest
import torch

import composite_ref as ref
import rasterize_ref as rref
from util import GRAD_TOL, rel_linf, scenes, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
MODULE_TOL = 1e-3       # two fp32 routes to one quantity (test_gpu_prep.py)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shifted(a):
    """``a`` on the GPU as a contiguous view that starts 4 bytes into its storage: no 16-byte alignment, the scalar paths."""
    if a is None:
        return None
    t = _cu(a)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _inputs(c, put=_cu):
    return put(c["values"]), put(c["alpha"]), put(c["render_layers"]), _cu(c["background"])


def _check_forward(c, what, put=_cu):
    """out, acc, final_T and n_contrib of the C entry point bit-equal to forward32's."""
    out, acc, fT, n = (x.cpu().numpy() for x in _C.composite_cuda(*_inputs(c, put)))
    assert out.shape == c["out"].shape and out.dtype == np.float32 and n.dtype == np.int32, what
    assert np.array_equal(n, c["n_contrib"]), (what, int((n != c["n_contrib"]).sum()))
    assert np.array_equal(_bits(fT), _bits(c["final_T"])), what
    assert np.array_equal(_bits(acc), _bits(f32(1) - c["final_T"])), what
    assert np.array_equal(_bits(out), _bits(c["out"])), (what, int((_bits(out) != _bits(c["out"])).sum()))
    return out


def _raw_backward(c, use_g=True, use_gA=True, need_v=True, need_a=True, put=_cu):
    """dm2_composite_backward through the C entry point into NaN-filled buffers (the per-face dL_dalpha zero-filled, as the
    contract asks of the caller) -> (dvalues or None, dalpha or None) as numpy."""
    lib = _C.load_library()
    v, a, rl, bg = _inputs(c, put)
    B, H, W, L, C = c["values"].shape
    per_face = c["alpha"].ndim == 1
    F = c["alpha"].shape[0] if per_face else 0
    g, gA = (put(c["g"]) if use_g else None), (_cu(c["gA"]) if use_gA else None)
    nc = _cu(c["n_contrib"])
    dv = torch.full((B, H, W, L, C), float("nan"), device="cuda") if need_v else None
    if put is _shifted and dv is not None:
        dv = _shifted(dv.cpu().numpy())
    da = None
    if need_a:
        da = torch.zeros(F, device="cuda") if per_face else torch.full((B, H, W, L), float("nan"), device="cuda")
    p = _C._ptr
    rc = lib.dm2_composite_backward(B, H, W, L, C, F, 1 if per_face else 0, p(v), p(a), p(rl), p(bg), p(nc), p(g), p(gA), p(dv), p(da),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dm2_last_error()
    torch.cuda.synchronize()
    return (None if dv is None else dv.cpu().numpy()), (None if da is None else da.cpu().numpy())


def _close(got, want, what):
    """Within GRAD_TOL relative L-inf; a reference that is zero everywhere must be met exactly."""
    assert got.shape == want.shape and np.isfinite(got).all(), what            # every element written (the buffers held NaN)
    if not want.any():
        assert not got.any(), what
        return 0.0
    e = rel_linf(got, want)
    assert e <= GRAD_TOL, (what, e)
    return e


def _check_grads(c, what, put=_cu):
    """g only, gA only, both; with both, each output gradient requested alone as well."""
    worst = 0.0
    per_face = c["alpha"].ndim == 1
    for use_g, use_gA in ((True, False), (False, True), (True, True)):
        wv, wa = ref.grads64(c["values"], c["alpha"], c["render_layers"], c["background"], c["n_contrib"],
                             c["g"] if use_g else None, c["gA"] if use_gA else None)
        assert np.abs(wa).max() > 0 and (np.abs(wv).max() > 0) == use_g, what
        dv, da = _raw_backward(c, use_g, use_gA, put=put)
        worst = max(worst, _close(dv, wv, (what, use_g, use_gA, "dvalues")), _close(da, wa, (what, use_g, use_gA, "dalpha")))
        assert not dv[~c["blend"]].any(), what                                  # zeros, exactly, in empty slots and behind the stop
        if not per_face:
            assert not da[~c["blend"]].any(), what
        if use_g and use_gA:
            dv1, none = _raw_backward(c, need_a=False, put=put)
            none2, da1 = _raw_backward(c, need_v=False, put=put)
            assert none is None and none2 is None
            assert np.array_equal(_bits(dv1), _bits(dv)), what                  # pure functions of the inputs
            if per_face:
                _close(da1, wa, (what, "dalpha alone"))
            else:
                assert np.array_equal(_bits(da1), _bits(da)), what
    return worst


@pytest.mark.parametrize("L", ref.LS)
def test_forward_bit_equal_to_restatement(L):
    """Every C at this L: a per-slot alpha with render_layers and a background and with neither, a per-face alpha with and
    without a background; where four-wide loads apply (L or C a multiple of 4) also from views 4 bytes into their storage: the
    scalar paths, the same bits."""
    for C in ref.CS:
        for per_face, layers, bg in ((False, True, True), (False, False, False), (True, True, True), (True, True, False)):
            c = ref.case(L, C, per_face, layers, bg, keep=False)
            _check_forward(c, (L, C, per_face, layers, bg))
            if L % 4 == 0 or C % 4 == 0:
                _check_forward(c, (L, C, per_face, layers, bg, "unaligned"), put=_shifted)


GRAD_GRID = [(L, ref.CS[i % len(ref.CS)], ref.CS[(i + 3) % len(ref.CS)]) for i, L in enumerate(ref.LS)]


def test_gradient_grid_covers_every_channel_count():
    assert {c for _, c1, c2 in GRAD_GRID for c in (c1, c2)} == set(ref.CS)


@pytest.mark.parametrize("L,C1,C2", GRAD_GRID)
def test_gradients_against_float64(L, C1, C2):
    """Per-slot alpha at C1 (render_layers given) and C2 (None), per-face alpha at C2; background given and None."""
    for C, per_face, layers, bg in ((C1, False, True, True), (C2, False, False, False), (C2, True, True, True), (C1, True, True, False)):
        c = ref.case(L, C, per_face, layers, bg)
        print(L, C, per_face, layers, bg, _check_grads(c, (L, C, per_face, layers, bg)))


@pytest.mark.parametrize("L,C", [(4, 4), (8, 16), (16, 4), (5, 16)])
def test_unaligned_tensors_give_the_same_gradients(L, C):
    for per_face in (False, True):
        c = ref.case(L, C, per_face)
        dv, da = _raw_backward(c)
        dvu, dau = _raw_backward(c, put=_shifted)
        assert np.array_equal(_bits(dv), _bits(dvu))
        if per_face:
            assert rel_linf(dau, da) <= GRAD_TOL
        else:
            assert np.array_equal(_bits(da), _bits(dau))
        _check_grads(c, ("unaligned", L, C, per_face), put=_shifted)


@pytest.mark.parametrize("L,C", [(5, 3), (8, 4), (17, 16)])
def test_nonfinite_data_in_slots_that_take_no_part(L, C):
    """NaN and inf in the values and alphas of empty slots and of slots behind the stop: outputs and gradients are finite and
    the same bits as without (the per-face dL/dalpha, summed with atomics: within GRAD_TOL)."""
    for per_face in (False, True):
        c = ref.case(L, C, per_face)
        d = dict(c)
        dead = ~c["blend"]
        v = c["values"].copy()
        v[dead] = np.where(np.arange(int(dead.sum()))[:, None] % 2 == 0, np.nan, np.inf).astype(f32)
        d["values"] = v
        if per_face:
            rl = c["render_layers"].copy()
            behind = dead & (rl >= 0) & (rl < c["alpha"].shape[0])
            rl[behind] = np.where(np.arange(int(behind.sum())) % 2 == 0, 2 ** 31 - 1, -2 ** 31).astype(np.int32)   # far outside the table
            d["render_layers"] = rl
            assert behind.any()
        else:
            a = c["alpha"].copy()
            a[dead] = np.where(np.arange(int(dead.sum())) % 3 == 0, np.inf, np.nan).astype(f32)
            d["alpha"] = a
        assert dead.mean() > 0.2
        out = _check_forward(d, ("planted", L, C, per_face))
        assert np.isfinite(out).all()
        dv0, da0 = _raw_backward(c)
        dv1, da1 = _raw_backward(d)
        assert np.isfinite(dv1).all() and np.isfinite(da1).all()
        assert np.array_equal(_bits(dv0), _bits(dv1))
        if per_face:
            wa = ref.grads64(c["values"], c["alpha"], c["render_layers"], c["background"], c["n_contrib"], c["g"], c["gA"])[1]
            assert rel_linf(da1, wa) <= GRAD_TOL
        else:
            assert np.array_equal(_bits(da0), _bits(da1))


def test_a_blended_slot_with_alpha_zero_still_adds():
    """inf in the values of blended slots whose alpha is exactly 0: inf * 0 = NaN reaches exactly the pixels the restatement
    says, and every other pixel keeps its bits."""
    c = ref.case(5, 3, False)
    zero = c["blend"] & (c["alpha"] == 0)
    v = c["values"].copy()
    v[zero] = np.inf
    want = ref.forward32(v, c["alpha"], c["render_layers"], c["background"])[0]
    out = _C.composite_cuda(_cu(v), *_inputs(c)[1:])[0].cpu().numpy()
    hit = zero.any(-1)
    assert hit.sum() > 100 and np.isnan(want[hit]).all()
    assert np.array_equal(np.isnan(out), np.isnan(want))
    assert np.array_equal(_bits(out[~hit]), _bits(c["out"][~hit]))


def test_the_stop_is_strictly_below_T_EPS():
    """Pixels whose transmittance lands on T_EPS exactly: 1 - a1 = 8192 T_EPS and 1 - a2 = 2^-13 are exact in float32 and so is
    their product.  T < T_EPS is false there, so the third slot still blends (n_contrib = 3, where T <= T_EPS would give 2); with the first two slots in the
    other order as well, and one step below and above T_EPS next to them."""
    x = ref.T_EPS * f32(8192)
    a1, a2 = f32(1) - x, f32(1) - f32(2.0 ** -13)
    assert f32(1) - a1 == x and (f32(1) - a1) * (f32(1) - a2) == ref.T_EPS
    rng = np.random.default_rng(17)
    shape, C = (1, 20, 30, 4), 3
    alpha = np.empty(shape, f32)
    alpha[..., 0], alpha[..., 1], alpha[..., 2:] = a1, a2, f32(0.25)
    alpha[:, 5:10, :, :2] = alpha[:, 5:10, :, 1::-1]
    alpha[:, 10:15, :, 0] = f32(1) - np.nextafter(x, f32(0))               # T one ulp below T_EPS: stops after two slots
    alpha[:, 15:, :, 0] = f32(1) - np.nextafter(x, f32(1))                 # one ulp above: goes on
    c = dict(values=rng.standard_normal(shape + (C,), dtype=f32), alpha=alpha, render_layers=None,
             background=rng.uniform(0, 1, C).astype(f32))
    c["out"], c["final_T"], c["n_contrib"], c["blend"] = ref.forward32(c["values"], alpha, None, c["background"], full=True)
    n = c["n_contrib"]
    assert (n[:, :10] == 3).all() and (n[:, 10:15] == 2).all() and (n[:, 15:] == 3).all()
    _check_forward(c, "T == T_EPS")


@pytest.mark.parametrize("name", sorted(ref.CROWDED))
def test_face_table_overflow_route(name):
    c = ref.crowded(name)
    lo, hi = ref.check_crowded(name, c, table_capacity())
    print(name, "distinct blended faces per tile", lo, hi)
    _check_forward(c, name)
    print(name, _check_grads(c, name))


def _soup():
    """rasterize_ref.scene("soup") as a scene on the GPU (the same generator call) -> (renderer, view indices, scene)."""
    sc = scenes.triangle_soup(90, 70, 1000, scenes.SEED_BASE + 80, num_cams=3, depth_complexity=30.0, shared_verts=True).to("cuda")
    s = rref.scene("soup")
    assert np.array_equal(sc.verts.cpu().numpy(), s["verts"]) and np.array_equal(sc.faces.cpu().numpy(), s["faces"])
    return dm2.LayeredRenderer(sc.mv, sc.proj, 90, 70, "cuda"), [2, 0, 2], sc


def test_module_path_end_to_end():
    """rasterize -> interpolate(UV) -> texture -> composite(faces_opacity) on the soup, L = 4, a 64 x 64 x 3 texture, a loss over
    out and acc.  composite's own input gradients against grads64 at GRAD_TOL; tex.grad, the UV table's, faces_opacity.grad and
    verts.grad against the same pipeline ending in the torch line (opacities <= 0.9: no pixel stops, one function) at 1e-3."""
    r, bidx, sc = _soup()
    assert type(r).composite is dm2.Renderer.composite                    # inherited
    L, F = 4, sc.faces.shape[0]
    gen = torch.Generator().manual_seed(21)
    table0 = (torch.rand((sc.verts.shape[0], 2), generator=gen) * 2 - 0.5).cuda()
    tex0 = torch.randn((64, 64, 3), generator=gen).cuda()
    op0 = (torch.rand(F, generator=gen) * 0.85 + 0.05).cuda()
    bg = torch.tensor([0.2, 0.5, 0.9]).cuda()
    wo, wa = None, None
    res = {}
    for route in ("op", "torch"):
        verts, table, tex, op = (x.clone().requires_grad_(True) for x in (sc.verts, table0, tex0, op0))
        layers, cnt, bary, t = r.rasterize(bidx, verts, sc.faces, L)
        uv = r.interpolate(layers, bary, table, sc.faces)
        values = r.texture(uv, tex, layers)
        values.retain_grad()
        out, acc = r.composite(values, op, layers, bg) if route == "op" else ref.one_liner(values, op, layers, bg)
        if wo is None:
            wo, wa = torch.randn(out.shape, generator=gen).cuda(), torch.randn(acc.shape, generator=gen).cuda()
        ((out * wo).sum() + (acc * wa).sum()).backward()
        res[route] = dict(out=out.detach(), acc=acc.detach(), values=values.detach(), dvalues=values.grad, layers=layers,
                          grads=dict(tex=tex.grad, table=table.grad, opacity=op.grad, verts=verts.grad))
    a, b = res["op"], res["torch"]
    assert int((a["layers"] >= 0).sum()) > 50_000 and torch.equal(a["values"], b["values"])
    vn, rl, on, bn = a["values"].cpu().numpy(), a["layers"].cpu().numpy(), op0.cpu().numpy(), bg.cpu().numpy()
    want_out, want_T, want_n = ref.forward32(vn, on, rl, bn)
    assert (want_T >= ref.T_EPS).all()                                    # no pixel stops: the torch line computes the same function
    assert np.array_equal(_bits(a["out"].cpu().numpy()), _bits(want_out))
    assert np.array_equal(_bits(a["acc"].cpu().numpy()), _bits(f32(1) - want_T))
    gv, ga = ref.grads64(vn, on, rl, bn, want_n, wo.cpu().numpy(), wa.cpu().numpy())
    ev, ea = rel_linf(a["dvalues"].cpu().numpy(), gv), rel_linf(a["grads"]["opacity"].cpu().numpy(), ga)
    print("composite's own: dvalues", ev, "dalpha", ea)
    assert np.abs(gv).max() > 0 and np.abs(ga).max() > 0 and ev <= GRAD_TOL and ea <= GRAD_TOL
    errs = {k: rel_linf(a["grads"][k].cpu().numpy(), b["grads"][k].cpu().numpy()) for k in a["grads"]}
    print("against the torch line:", errs)
    assert all(float(b["grads"][k].abs().max()) > 0 for k in errs)
    assert all(e <= MODULE_TOL for e in errs.values()), errs


@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("name", ["soup", "lattice", "degenerate"])
def test_composite_of_interpolated_colours_is_render(name, L):
    """rasterize's layers through LayeredRenderer.render (faces_intense = 1) against interpolate(verts_color) -> composite: alpha
    (1 - final_T) bit-equal, colour within 1e-6 absolute, no pixel excused (the CPU test's bars; n_contrib is not an output of
    render)."""
    s = rref.scene(name)
    P, F, B = s["verts"].shape[0], s["faces"].shape[0], s["verts_ndc"].shape[0]
    tab = ref.render_tables(P, F, B, L)
    color, op, bg = _cu(tab["color"]), _cu(tab["opacity"]), _cu(tab["background"])
    verts, faces = _cu(s["verts"]), _cu(s["faces"])
    layers, cnt, bary, t = _C.rasterize_layers_cuda(s["W"], s["H"], verts, faces, None, _cu(s["verts_ndc"]), _cu(s["verts_image"]),
                                                    _cu(s["ray_o"]), _cu(s["ray_d"]), L)
    want = _C.composite_layers_cuda(layers, verts, faces, color, op, torch.ones((B, F), device="cuda"), _cu(s["verts_ndc"]), bg,
                                    _cu(s["ray_o"]), _cu(s["ray_d"]))
    want_color, want_T, want_n = want[0], want[2], want[3]
    values = _C.interpolate_cuda(layers, bary, color, faces)
    out, acc, fT, n = _C.composite_cuda(values, op, layers, bg)
    assert float((n > 0).float().mean()) > 0.2 and int((fT < float(ref.T_EPS)).sum()) > 4
    assert torch.equal(fT, want_T) and torch.equal(acc, 1.0 - want_T) and torch.equal(n, want_n)
    err = float((out - want_color).abs().max())
    print(name, L, "colour", err)
    assert err <= 1e-6


def test_render_method_agrees_with_composite():
    """The same through the public methods: LayeredRenderer.render(return_alpha=True) against rasterize -> interpolate -> composite."""
    r, bidx, sc = _soup()
    F = sc.faces.shape[0]
    gen = torch.Generator().manual_seed(22)
    op = torch.rand(F, generator=gen).cuda()
    op[::7] = 1.0
    color = torch.rand((sc.verts.shape[0], 3), generator=gen).cuda()
    bg = torch.tensor([0.2, 0.5, 0.9]).cuda()
    with torch.no_grad():
        layers, cnt, bary, t = r.rasterize(bidx, sc.verts, sc.faces, 4)
        want_color, _, want_alpha = r.render(bidx, layers, sc.verts, sc.faces, color, op, torch.ones((3, F), device="cuda"), bg,
                                             return_alpha=True)
        out, acc = r.composite(r.interpolate(layers, bary, color, sc.faces), op, layers, bg)
    assert float((acc > 0).float().mean()) > 0.2 and torch.equal(acc, want_alpha)
    assert float((out - want_color).abs().max()) <= 1e-6


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


@pytest.mark.parametrize("per_face", [False, True])
def test_side_stream(per_face):
    """The inputs are produced on a side stream only, behind a delay (asynchronous copies from pinned memory into tensors that
    hold another case's data); forward and backward run there and nothing but that stream is waited for.  A launch that went to
    another stream would read the other case."""
    c, other = ref.case(9, 3, per_face), ref.case(9, 3, per_face, bg=False)
    keys = ("values", "alpha", "render_layers", "background", "g", "gA")
    host = {k: torch.from_numpy(c[k]).pin_memory() for k in keys}
    rng = np.random.default_rng(5)
    poison = dict(values=other["values"][::-1].copy(), alpha=rng.permutation(c["alpha"].reshape(-1)).reshape(c["alpha"].shape),
                  render_layers=other["render_layers"][::-1].copy(), background=1 - c["background"], g=-c["g"], gA=c["gA"][::-1].copy())
    wv, wa = ref.grads64(c["values"], c["alpha"], c["render_layers"], c["background"], c["n_contrib"], c["g"], c["gA"])
    for side in (torch.cuda.Stream(), torch.cuda.Stream()):
        dev = {k: _cu(poison[k]) for k in keys}
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            d1 = _Delay(side)
            for k in keys:
                dev[k].copy_(host[k], non_blocking=True)
            v, a = dev["values"].requires_grad_(True), dev["alpha"].requires_grad_(True)
            out, acc = dm2.CompositeFunction.apply(v, a, dev["render_layers"], dev["background"])
            ((out * dev["g"]).sum() + (acc * dev["gA"]).sum()).backward()
            side.synchronize()
            got = [x.detach().cpu().numpy() for x in (out, acc, v.grad, a.grad)]
        assert np.array_equal(_bits(got[0]), _bits(c["out"])) and np.array_equal(_bits(got[1]), _bits(f32(1) - c["final_T"]))
        assert rel_linf(got[2], wv) <= GRAD_TOL and rel_linf(got[3], wa) <= GRAD_TOL
        d1.check()
        for k in keys:
            dev[k].grad = None
    torch.cuda.synchronize()


def test_needs_input_grad_and_missing_output_gradients():
    c = ref.case(4, 3, True)
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    calls, launches = [], []
    real = _C.composite_backward_cuda
    lib = _C.load_library()
    real_b = lib.dm2_composite_backward

    def spy(*args):
        calls.append((args[5] is not None, args[6] is not None) + tuple(args[7:]))
        return real(*args)
    _C.composite_backward_cuda = spy
    lib.dm2_composite_backward = lambda *x: launches.append("b") or real_b(*x)
    try:
        wv, wa = ref.grads64(c["values"], c["alpha"], c["render_layers"], c["background"], c["n_contrib"], c["g"], None)
        for need_v, need_a in ((True, True), (True, False), (False, True)):
            v, a, rl, bg = _inputs(c)
            v.requires_grad_(need_v); a.requires_grad_(need_a)
            out, acc = r.composite(v, a, rl, bg)
            out.backward(_cu(c["g"]))                                     # acc is left out of the loss: its gradient arrives as None
            assert (v.grad is not None) == need_v and (a.grad is not None) == need_a
            if need_v:
                assert rel_linf(v.grad.cpu().numpy(), wv) <= GRAD_TOL
            if need_a:
                assert rel_linf(a.grad.cpu().numpy(), wa) <= GRAD_TOL
        assert calls == [(True, False, True, True), (True, False, True, False), (True, False, False, True)] and len(launches) == 3
        v, a, rl, bg = _inputs(c)
        v.requires_grad_(True)
        out, acc = r.composite(v, a, rl, bg)
        acc.sum().backward()                                               # gA alone: dL/dvalues is zero, and written
        assert calls[-1] == (False, True, True, False) and not v.grad.any()
        del calls[:], launches[:]
        # neither output in the loss, or no input that requires grad: no call, no launch
        v, a, rl, bg = _inputs(c)
        v.requires_grad_(True)
        out, acc = r.composite(v, a, rl, bg)
        (v.sum() + 0 * out.detach().sum()).backward()
        out2, acc2 = r.composite(*_inputs(c))
        assert out2.grad_fn is None and acc2.grad_fn is None
        assert real(*_inputs(c), _cu(c["n_contrib"]), None, None, True, True) == (None, None)
        assert real(*_inputs(c), _cu(c["n_contrib"]), _cu(c["g"]), None, False, False) == (None, None)
        assert not calls and not launches
    finally:
        _C.composite_backward_cuda = real
        lib.dm2_composite_backward = real_b


def test_argument_checks():
    v = torch.zeros((2, 4, 5, 3, 6), device="cuda")
    a = torch.zeros((2, 4, 5, 3), device="cuda")
    af = torch.zeros(7, device="cuda")
    rl = torch.zeros((2, 4, 5, 3), dtype=torch.int32, device="cuda")
    bg = torch.zeros(6, device="cuda")
    out, acc, fT, n = _C.composite_cuda(v, a, rl, bg)
    assert tuple(out.shape) == (2, 4, 5, 6) and tuple(acc.shape) == (2, 4, 5) and n.dtype == torch.int32
    assert tuple(_C.composite_cuda(v, af, rl)[0].shape) == (2, 4, 5, 6)
    for args, name in (((v[0], a, rl, bg), "values"), ((v[..., :0], a, rl, bg[:0]), "values"), ((v.double(), a, rl, bg), "values"),
                       ((v, a[:1], rl, bg), "alpha"), ((v, a[0], rl, bg), "alpha"), ((v, a.half(), rl, bg), "alpha"),
                       ((v, af, None, bg), "render_layers"), ((v, a, rl[..., :2], bg), "render_layers"),
                       ((v, a, rl.long(), bg), "render_layers"), ((v, a, rl, bg[:3]), "background"),
                       ((v, a, rl, bg[None]), "background"), ((v, a, rl, bg.double()), "background")):
        with pytest.raises(RuntimeError, match=name):
            _C.composite_cuda(*args)
    with pytest.raises(RuntimeError, match="grad_out"):
        _C.composite_backward_cuda(v, a, rl, bg, n, out[..., :2], None, True, True)
    with pytest.raises(RuntimeError, match="grad_acc"):
        _C.composite_backward_cuda(v, a, rl, bg, n, out, acc[0], True, True)
    with pytest.raises(RuntimeError, match="n_contrib"):
        _C.composite_backward_cuda(v, a, rl, bg, n[0], out, acc, True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.composite_cuda(v.cpu(), a.cpu(), rl.cpu(), bg.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.composite_cuda(v, a.cpu(), rl, bg)
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    with pytest.raises(RuntimeError, match="render_layers"):
        r.composite(v, af)
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    p = _C._ptr
    assert lib.dm2_composite(2, 4, 5, 3, 6, 0, 0, p(v), p(a), p(rl), p(bg), p(out), p(acc), p(fT), p(n), None) == 0
    assert lib.dm2_composite(2, 4, 5, 3, 6, 0, 2, p(v), p(a), p(rl), p(bg), p(out), p(acc), p(fT), p(n), None) == 1
    assert lib.dm2_composite(2, 4, 5, 3, 0, 0, 0, p(v), p(a), p(rl), p(bg), p(out), p(acc), p(fT), p(n), None) == 1
    assert lib.dm2_composite(2, 4, 5, 3, 6, 7, 1, p(v), p(af), None, p(bg), p(out), p(acc), p(fT), p(n), None) == 1
    assert lib.dm2_composite(2, 4, 5, 3, 6, 0, 0, None, p(a), p(rl), p(bg), p(out), p(acc), p(fT), p(n), None) == 1
    assert lib.dm2_composite(2, 4, 5, 3, 6, 0, 0, p(v), p(a), p(rl), p(bg), None, p(acc), p(fT), p(n), None) == 1
    assert lib.dm2_composite_backward(2, 4, 5, 3, 6, 0, 0, p(v), p(a), p(rl), p(bg), None, p(out), None, p(v), None, None) == 1
    torch.cuda.synchronize()


def test_degenerate_sizes():
    """B * H * W == 0 or L == 0: T = 1 everywhere, out = background (or zeros), acc = 0, without entering the library; through the
    C entry point L == 0 gives the same."""
    bg = torch.tensor([0.25, 0.5, 0.75], device="cuda")
    launches = []
    lib = _C.load_library()
    real_f, real_b = lib.dm2_composite, lib.dm2_composite_backward
    try:
        lib.dm2_composite = lambda *x: launches.append("f") or real_f(*x)
        lib.dm2_composite_backward = lambda *x: launches.append("b") or real_b(*x)
        for shape in ((0, 4, 5, 2), (2, 0, 5, 2), (2, 4, 0, 2), (2, 4, 5, 0)):
            v = torch.zeros(shape + (3,), device="cuda")
            rl = torch.zeros(shape, dtype=torch.int32, device="cuda")
            for alpha in (torch.zeros(shape, device="cuda"), torch.zeros(9, device="cuda")):
                for b in (bg, None):
                    out, acc, fT, n = _C.composite_cuda(v, alpha, rl, b)
                    assert tuple(out.shape) == shape[:3] + (3,) and tuple(acc.shape) == shape[:3]
                    assert torch.equal(out, (bg if b is not None else torch.zeros(3, device="cuda")).expand(shape[:3] + (3,)))
                    assert not acc.any() and not n.any() and (fT == 1).all()
                    dv, da = _C.composite_backward_cuda(v, alpha, rl, b, n, torch.ones_like(out), torch.ones_like(acc), True, True)
                    assert tuple(dv.shape) == tuple(v.shape) and tuple(da.shape) == tuple(alpha.shape) and not da.any()
        assert not launches
    finally:
        lib.dm2_composite, lib.dm2_composite_backward = real_f, real_b
    out = torch.full((2, 4, 5, 3), float("nan"), device="cuda")
    acc, fT = torch.full((2, 4, 5), float("nan"), device="cuda"), torch.full((2, 4, 5), float("nan"), device="cuda")
    n = torch.full((2, 4, 5), 7, dtype=torch.int32, device="cuda")
    p = _C._ptr
    assert lib.dm2_composite(2, 4, 5, 0, 3, 0, 0, None, None, None, p(bg), p(out), p(acc), p(fT), p(n), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, bg.expand(2, 4, 5, 3)) and not acc.any() and (fT == 1).all() and not n.any()


def test_full_size():
    """1920 x 1080, L = 4, C = 3, a per-face alpha: forward and backward.  (B H W L C = 2.5e7: below 2^31 elements.)"""
    rng = np.random.default_rng(9)
    shape, C, F = (1, 1080, 1920, 4), 3, 200_000
    ys, xs = np.meshgrid(np.arange(1080) // 8, np.arange(1920) // 8, indexing="ij")
    rl = (((ys * 240 + xs)[None, :, :, None] * 7 + np.arange(4) * 50_021 + rng.integers(0, 3, shape)) % F).astype(np.int32)
    rl[rng.uniform(size=shape) < 0.2] = -1                                 # (neighbouring pixels list neighbouring faces, as a mesh does)
    alpha = rng.uniform(0, 1, F).astype(f32)
    alpha[::11] = 1.0
    alpha[5::11] = 0.0
    c = dict(values=rng.standard_normal(shape + (C,), dtype=f32), alpha=alpha, render_layers=rl,
             background=np.array([0.2, 0.5, 0.9], f32), g=rng.standard_normal(shape[:3] + (C,), dtype=f32),
             gA=rng.standard_normal(shape[:3], dtype=f32))
    c["out"], c["final_T"], c["n_contrib"], c["blend"] = ref.forward32(c["values"], alpha, rl, c["background"], full=True)
    assert (c["final_T"] < ref.T_EPS).mean() > 0.05 and c["blend"].mean() > 0.5
    _check_forward(c, "full size")
    wv, wa = ref.grads64(c["values"], alpha, rl, c["background"], c["n_contrib"], c["g"], c["gA"])
    dv, da = _raw_backward(c)
    ev, ea = _close(dv, wv, "full size dvalues"), _close(da, wa, "full size dalpha")
    print("full size dvalues", ev, "dalpha", ea)
    assert not dv[~c["blend"]].any()
