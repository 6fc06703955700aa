"""Renderer.interpolate / dm2_interpolate on the GPU against the contract's restatement (tests/interpolate_ref.py): the forward
bit-equal to forward32, both gradients within GRAD_TOL of grads64; the table-overflow route of the attr scatter; ids and
attr_faces rows out of range; needs_input_grad; the module path from rasterize to verts.grad; one full-size case."""
import numpy as np
import pytest
import torch

import interpolate_ref as ref
import rasterize_ref as rref
from util import GRAD_TOL, rel_linf, scenes, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

CS = (1, 2, 3, 4, 7, 16, 33)
LS = (1, 4, 8)
INT32_MIN = int(np.iinfo(np.int32).min)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_RAS = {}


def _rasterized(name, L):
    """rasterize_layers_cuda on rasterize_ref.scene(name): (scene, layers, bary) as numpy."""
    if (name, L) not in _RAS:
        s = rref.scene(name)
        layers, cnt, bary, t = _C.rasterize_layers_cuda(s["W"], s["H"], _cu(s["verts"]), _cu(s["faces"]), None, _cu(s["verts_ndc"]),
                                                        _cu(s["verts_image"]), _cu(s["ray_o"]), _cu(s["ray_d"]), L)
        _RAS[(name, L)] = (s, layers.cpu().numpy(), bary.cpu().numpy())
    return _RAS[(name, L)]


def _attr(rng, B, N, C, per_view):
    return rng.standard_normal((B, N, C) if per_view else (N, C)).astype(np.float32)


def _fwd(rl, bary, attr, af):
    out = _C.interpolate_cuda(_cu(rl), _cu(bary), _cu(attr), _cu(af))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bwd(rl, bary, attr, af, g, need_attr=True, need_bary=True):
    da, db = _C.interpolate_backward_cuda(_cu(rl), _cu(bary), _cu(attr), _cu(af), _cu(g), need_attr, need_bary)
    torch.cuda.synchronize()
    return (None if da is None else da.cpu().numpy()), (None if db is None else db.cpu().numpy())


def _check_forward(rl, bary, attr, af, what):
    got = _fwd(rl, bary, attr, af)
    want = ref.forward32(rl, bary, attr, af)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
    return got


def _check_grads(rl, bary, attr, af, g, what):
    da, db = _bwd(rl, bary, attr, af, g)
    wa, wb = ref.grads64(rl, bary, attr, af, g)
    assert da.shape == attr.shape and db.shape == bary.shape, what
    ea, eb = rel_linf(da, wa), rel_linf(db, wb)
    print(what, "dattr", ea, "dbary", eb)
    assert np.abs(wa).max() > 0 and np.abs(wb).max() > 0, what
    assert np.isfinite(da).all() and ea <= GRAD_TOL, (what, "dattr", ea)
    assert np.isfinite(db).all() and eb <= GRAD_TOL, (what, "dbary", eb)
    m, _ = ref.filled(rl, af, attr.shape[-2])
    assert (db[~m] == 0).all(), what
    return da, db


@pytest.mark.parametrize("name", rref.SCENES)
@pytest.mark.parametrize("L", LS)
def test_forward_bit_equal_to_restatement(name, L):
    s, rl, bary = _rasterized(name, L)
    B, P, F = rl.shape[0], s["verts"].shape[0], s["faces"].shape[0]
    rng = np.random.RandomState(100 + L)
    filled_slots = int((rl >= 0).sum())
    if L == 4:
        floor = {"soup": 50_000, "lattice": 15_000, "degenerate": 4_000, "no_faces": None}[name]
        assert filled_slots == 0 if floor is None else filled_slots > floor, (name, filled_slots)
    for C in CS:
        for per_view in (False, True):
            got = _check_forward(rl, bary, _attr(rng, B, P, C, per_view), s["faces"], (name, L, C, per_view))
            if name == "no_faces":
                assert got.shape == rl.shape + (C,) and (got == 0).all()
            else:
                assert 0.99 * filled_slots <= (np.abs(got).max(-1) > 0).sum() <= filled_slots
        # a table of its own (UV seams): N != P
        N = 2 * P + 5
        af = rng.randint(0, N, (F, 3)).astype(np.int32)
        _check_forward(rl, bary, _attr(rng, B, N, C, False), af, (name, L, C, "own table"))


@pytest.mark.parametrize("name", ["soup", "lattice"])
@pytest.mark.parametrize("L", LS)
def test_gradients_against_float64(name, L):
    s, rl, bary = _rasterized(name, L)
    B, P = rl.shape[0], s["verts"].shape[0]
    rng = np.random.RandomState(200 + L)
    for C in CS:
        for per_view in (False, True):
            attr = _attr(rng, B, P, C, per_view)
            g = rng.standard_normal(rl.shape + (C,)).astype(np.float32)
            _check_grads(rl, bary, attr, s["faces"], g, (name, L, C, per_view))


@pytest.mark.parametrize("C", [3, 16])
def test_table_overflow_route(C):
    """Hand-built layers with more distinct faces per 16 x 16 tile than the scatter's LDS table holds: the faces that find no
    slot add straight to global memory."""
    F, N, shape = 5000, 3000, (2, 48, 64, 4)
    rl = np.random.RandomState(5).randint(0, F, shape).astype(np.int32)
    least = ref.distinct_per_tile(rl)
    print("distinct ids per tile, at least", least)
    assert least > table_capacity()
    rng = np.random.RandomState(6)
    bary = rng.uniform(0, 1, shape + (3,)).astype(np.float32)
    af = rng.randint(0, N, (F, 3)).astype(np.int32)
    for per_view in (False, True):
        attr = _attr(rng, shape[0], N, C, per_view)
        g = rng.standard_normal(shape + (C,)).astype(np.float32)
        _check_forward(rl, bary, attr, af, ("overflow", C, per_view))
        _check_grads(rl, bary, attr, af, g, ("overflow", C, per_view))


@pytest.mark.parametrize("per_view", [False, True])
def test_out_of_range_ids_and_rows(per_view):
    s, rl, bary = _rasterized("soup", 4)
    B, P, F, C = rl.shape[0], s["verts"].shape[0], s["faces"].shape[0], 5
    rng = np.random.RandomState(7)
    rl_bad = rl.copy()
    hit = np.flatnonzero(rl.reshape(-1) >= 0)
    pick = rng.choice(hit, 4000, replace=False)
    rl_bad.reshape(-1)[pick] = np.array([F, F + 7, -5, INT32_MIN], np.int32)[np.arange(4000) % 4]
    af = s["faces"].copy()
    bad_faces = rng.choice(F, 60, replace=False)
    af[bad_faces, np.arange(60) % 3] = np.array([P, -1, P + 1000, INT32_MIN, np.iinfo(np.int32).max], np.int32)[np.arange(60) % 5]
    empty = np.zeros(rl.shape, bool)
    empty.reshape(-1)[pick] = True
    empty |= np.isin(rl, bad_faces)
    assert empty.sum() > 5000 and (rl[~empty] >= 0).sum() > 50_000
    rl_clean = np.where(empty, -1, rl).astype(np.int32)
    attr = _attr(rng, B, P, C, per_view)
    g = rng.standard_normal(rl.shape + (C,)).astype(np.float32)
    out = _check_forward(rl_bad, bary, attr, af, "bad ids")
    assert (out[empty] == 0).all()
    da, db = _check_grads(rl_bad, bary, attr, af, g, "bad ids")
    assert (db[empty] == 0).all()
    out_c = _fwd(rl_clean, bary, attr, s["faces"])
    da_c, db_c = _bwd(rl_clean, bary, attr, s["faces"], g)
    assert np.array_equal(_bits(out), _bits(out_c)) and np.array_equal(_bits(db), _bits(db_c))
    assert rel_linf(da, da_c) <= GRAD_TOL


def test_needs_input_grad():
    s, rl, bary = _rasterized("lattice", 4)
    P, C = s["verts"].shape[0], 6
    rng = np.random.RandomState(8)
    attr = _attr(rng, rl.shape[0], P, C, False)
    g = _cu(rng.standard_normal(rl.shape + (C,)).astype(np.float32))
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    calls = []
    real = _C.interpolate_backward_cuda

    def spy(*a):
        calls.append(tuple(a[-2:]))
        return real(*a)
    _C.interpolate_backward_cuda = spy
    try:
        res = {}
        for need_a, need_b in ((True, True), (True, False), (False, True)):
            a, b = _cu(attr).requires_grad_(need_a), _cu(bary).requires_grad_(need_b)
            out = r.interpolate(_cu(rl), b, a, _cu(s["faces"]))
            out.backward(g, retain_graph=True)
            first = None if a.grad is None else a.grad.clone()
            if need_a:
                a.grad = None
                out.backward(g)                                              # a second backward of the same forward
                assert rel_linf(a.grad.cpu().numpy(), first.cpu().numpy()) <= GRAD_TOL
            res[(need_a, need_b)] = (first, None if b.grad is None else b.grad.clone())
        assert calls == [(True, True), (True, True), (True, False), (True, False), (False, True)]
        assert res[(True, False)][1] is None and res[(False, True)][0] is None
        # the second backward accumulated into bary.grad: twice the first
        assert torch.equal(res[(True, True)][1], 2 * res[(False, True)][1])
        assert rel_linf(res[(True, False)][0].cpu().numpy(), res[(True, True)][0].cpu().numpy()) <= GRAD_TOL
        wa, wb = ref.grads64(rl, bary, attr, s["faces"], g.cpu().numpy())
        assert rel_linf(res[(True, False)][0].cpu().numpy(), wa) <= GRAD_TOL
        assert rel_linf(res[(False, True)][1].cpu().numpy(), wb) <= GRAD_TOL
        del calls[:]
        out = r.interpolate(_cu(rl), _cu(bary), _cu(attr), _cu(s["faces"]))
        assert out.grad_fn is None
        w = torch.ones(1, device="cuda", requires_grad=True)
        (out.sum() * w).backward()
        assert not calls
    finally:
        _C.interpolate_backward_cuda = real


@pytest.mark.parametrize("C", [4, 16])
def test_unaligned_tables_give_the_same_bits(C):
    """attr and the upstream gradient as views that start 4 bytes into their storage (no 16-byte alignment): the bary
    backward's four-channel reads do not apply; the results are the same bits as with aligned tensors."""
    s, rl, bary = _rasterized("soup", 4)
    P = s["verts"].shape[0]
    rng = np.random.RandomState(13)
    attr = _attr(rng, rl.shape[0], P, C, False)
    g = rng.standard_normal(rl.shape + (C,)).astype(np.float32)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = _cu(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    args = (_cu(rl), _cu(bary))
    out_a = _C.interpolate_cuda(*args, _cu(attr), _cu(s["faces"]))
    out_u = _C.interpolate_cuda(*args, shifted(attr), _cu(s["faces"]))
    da_a, db_a = _C.interpolate_backward_cuda(*args, _cu(attr), _cu(s["faces"]), _cu(g), True, True)
    da_u, db_u = _C.interpolate_backward_cuda(*args, shifted(attr), _cu(s["faces"]), shifted(g), True, True)
    assert torch.equal(out_a, out_u) and torch.equal(db_a, db_u)
    assert rel_linf(da_u.cpu().numpy(), da_a.cpu().numpy()) <= GRAD_TOL
    wa, wb = ref.grads64(rl, bary, attr, s["faces"], g)
    assert rel_linf(db_u.cpu().numpy(), wb) <= GRAD_TOL and rel_linf(da_u.cpu().numpy(), wa) <= GRAD_TOL


def test_degenerate_sizes():
    s, rl, bary = _rasterized("lattice", 4)
    P, F, C = s["verts"].shape[0], s["faces"].shape[0], 3
    attr = _attr(np.random.RandomState(9), rl.shape[0], P, C, False)
    launches = []
    lib = _C.load_library()
    real_f, real_b = lib.dm2_interpolate, lib.dm2_interpolate_backward
    cases = ((rl[..., :0], bary[..., :0, :], attr, s["faces"]), (rl, bary, attr, s["faces"][:0]), (rl, bary, attr[:0], s["faces"]),
             (rl[:, :0], bary[:, :0], attr, s["faces"]))
    try:
        lib.dm2_interpolate = lambda *a: launches.append("f") or real_f(*a)
        lib.dm2_interpolate_backward = lambda *a: launches.append("b") or real_b(*a)
        for a in cases:
            out = _C.interpolate_cuda(*[_cu(x) for x in a])
            assert tuple(out.shape) == a[0].shape + (C,) and (out == 0).all()
            g = torch.ones_like(out)
            da, db = _C.interpolate_backward_cuda(*[_cu(x) for x in a], g, True, True)
            assert tuple(da.shape) == a[2].shape and tuple(db.shape) == a[1].shape and (da == 0).all() and (db == 0).all()
        assert not launches
    finally:
        lib.dm2_interpolate, lib.dm2_interpolate_backward = real_f, real_b


def _module_scene(name, W, H):
    if name == "lattice":
        ts = scenes.tet_lattice(W, H, 4, seed=scenes.SEED_BASE + 84, num_cams=2).to("cuda")
        return ts.mv, ts.proj, ts.verts, ts.faces
    sc = scenes.triangle_soup(W, H, 600, scenes.SEED_BASE + 85, num_cams=2, depth_complexity=12.0, shared_verts=True).to("cuda")
    return sc.mv, sc.proj, sc.verts, sc.faces


@pytest.mark.parametrize("name", ["lattice", "soup"])
@pytest.mark.parametrize("analytic", [False, True])
def test_module_path_end_to_end(name, analytic):
    """rasterize -> interpolate -> a random-weighted sum: attr.grad and verts.grad against float64 (verts through
    rasterize_ref.grads64 fed this op's float64 dL/dbary), and against the torch one-liner on the same bary."""
    from oracle import cpu as orc
    W, H, bidx, L, C = 80, 64, [1, 0], 4, 5
    mv, proj, verts0, faces = _module_scene(name, W, H)
    r = dm2.Renderer(mv, proj, W, H, "cuda", analytic_rays=analytic)
    if analytic:
        cam = r.ray_cam.cpu().numpy()
        ro, rd = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), W, H)
        ro, rd = ro[bidx], rd[bidx]
    else:
        ro, rd = r._camera_rows(r.ray_o, bidx).cpu().numpy(), r._camera_rows(r.ray_d, bidx).cpu().numpy()
    gen = torch.Generator().manual_seed(11)
    attr0 = torch.randn((verts0.shape[0], C), generator=gen).cuda()
    verts, attr = verts0.clone().requires_grad_(True), attr0.clone().requires_grad_(True)
    layers, cnt, bary, t = r.rasterize(bidx, verts, faces, L)
    out = r.interpolate(layers, bary, attr, faces)
    wgt = torch.randn(out.shape, generator=gen).cuda()
    (out * wgt).sum().backward()
    assert int(cnt.sum()) > 3000
    rl, bn, an, fn, gn = (x.detach().cpu().numpy() for x in (layers, bary, attr0, faces, wgt))
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(ref.forward32(rl, bn, an, fn)))
    wa, wb = ref.grads64(rl, bn, an, fn, gn)
    wv = rref.grads64(verts0.cpu().numpy(), fn, rl, ro, rd, wb, None)
    ea, ev = rel_linf(attr.grad.cpu().numpy(), wa), rel_linf(verts.grad.cpu().numpy(), wv)
    print(name, analytic, "attr.grad", ea, "verts.grad", ev)
    assert np.abs(wa).max() > 0 and np.abs(wv).max() > 0
    assert ea <= GRAD_TOL and ev <= GRAD_TOL
    # the torch one-liner on the same bary
    verts_t, attr_t = verts0.clone().requires_grad_(True), attr0.clone().requires_grad_(True)
    layers_t, _, bary_t, _ = r.rasterize(bidx, verts_t, faces, L)
    assert torch.equal(layers_t, layers) and torch.equal(bary_t, bary)
    (ref.one_liner(layers_t, bary_t, attr_t, faces) * wgt).sum().backward()
    ea, ev = rel_linf(attr.grad.cpu().numpy(), attr_t.grad.cpu().numpy()), rel_linf(verts.grad.cpu().numpy(), verts_t.grad.cpu().numpy())
    print(name, analytic, "against the one-liner: attr.grad", ea, "verts.grad", ev)
    assert ea <= GRAD_TOL and ev <= GRAD_TOL


def test_cfg3_full_size():
    """SURVEY.md 8(d) cfg 3: tet_lattice(n=25) at 1024^2, L = 4, C = 3."""
    ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to("cuda")
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, "cuda")
    with torch.no_grad():
        layers, cnt, bary, t = lr.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
    gen = torch.Generator().manual_seed(12)
    attr = torch.randn((ts.verts.shape[0], 3), generator=gen).cuda().requires_grad_(True)
    out = lr.interpolate(layers, bary, attr, ts.faces)
    g = torch.randn(out.shape, generator=gen).cuda()
    out.backward(g)
    rl, bn, an, fn = (x.detach().cpu().numpy() for x in (layers, bary, attr, ts.faces))
    assert int((rl >= 0).sum()) > 500_000
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(ref.forward32(rl, bn, an, fn)))
    wa, _ = ref.grads64(rl, bn, an, fn, g.cpu().numpy())
    e = rel_linf(attr.grad.cpu().numpy(), wa)
    print("cfg3 dattr", e)
    assert np.abs(wa).max() > 0 and e <= GRAD_TOL
