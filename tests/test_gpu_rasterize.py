"""Renderer.rasterize / dm2_rasterize_run on the GPU against the contract's restatement (tests/rasterize_ref.py): ids, counts,
barycentrics and t bit-equal, gradients within GRAD_TOL of float64 autograd; analytic rays; agreement with generate and,
through LayeredRenderer.render, with Renderer at aa_temperature 0; the backward's face-table overflow route; the module path."""
import numpy as np
import pytest
import torch

import rasterize_ref as ref
from util import GRAD_TOL, rel_linf, scenes, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

OUTS = ("layers", "cnt", "bary", "t")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _dev(s, fe):
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return (s["W"], s["H"], c(s["verts"]), c(s["faces"]), None if fe is None else c(fe), c(s["verts_ndc"]), c(s["verts_image"]),
            c(s["ray_o"]), c(s["ray_d"]))


def _equal(got, want, what):
    for k, g in zip(OUTS, got):
        g = g.cpu().numpy()
        assert g.shape == want[k].shape, (what, k, g.shape, want[k].shape)
        assert np.array_equal(_bits(g), _bits(want[k])), (what, k, int((_bits(g) != _bits(want[k])).sum()))


_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = ref.scene(name)
    return _SCENES[name]


@pytest.mark.parametrize("name", ref.SCENES)
@pytest.mark.parametrize("L", [0, 1, 2, 3, 5, 8, 12, 16, 17, 32, 33, 40])
@pytest.mark.parametrize("exist", [False, True])
def test_op_bit_equal_to_restatement(name, L, exist):
    """L = 1, 2, 3, 8, 16: k_rasterize<1, 2, 4, 8, 16> with full register lists; 5 and 12: lists of 8 and 16 slots of which
    only L are used; 17, 33: a last pass of one slot after one or two full ones; 32: a list that ends on a pass boundary."""
    s = _scene(name)
    fe = s["fe"] if exist else None
    got = _C.rasterize_layers_cuda(*_dev(s, fe), L)
    torch.cuda.synchronize()
    want = ref.rasterize32(s["W"], s["H"], s["verts"], s["faces"], fe, s["verts_ndc"], s["verts_image"], s["ray_o"], s["ray_d"], L)
    _equal(got, want, (name, L, exist))
    if name == "soup" and L > 16:
        assert (want["cnt"] > (32 if L == 40 and not exist else 16)).any()      # (the later passes had work)
    if name == "soup" and not exist and L in (2, 5, 12, 32, 33):
        assert (want["cnt"] == L).any()                                         # (some pixel fills every slot)


TET_BIT = ("aligned", "holes", "inside", "flat", "duplicates", "deep", "chunk_edge", "chunk_edge3")
DEEP_SORT_SIZE = (16, 16)        # (test_rasterize_cpu.py's: the reference is shared within one run)


@pytest.mark.parametrize("name", TET_BIT)
@pytest.mark.parametrize("L", [1, 4, 16, 17, 33, 40])
@pytest.mark.parametrize("exist", [None, "fe", "fe_odd"])
def test_op_bit_equal_on_tet_scenes(name, L, exist):
    """The tet scenes (rasterize_ref.tet_case; what each reaches is counted in test_rasterize_cpu.py): rays in face planes,
    through vertices and along edges (aligned: the hit rule, exact-edge hits), exact t ties that the face id decides, within
    a pass and across the pass boundaries 15|16 and 31|32 (duplicates, flat, aligned), cameras inside the mesh (inside,
    holes), lists of 40 staging chunks with hits for three passes (deep), a list that ends one entry into a chunk
    (chunk_edge, chunk_edge3); existence values other than 0 / 1 (fe_odd: 2, -1, INT_MIN)."""
    s = ref.tet_case(name)
    want = ref.select(ref.tet_intersect(name, exist), L)
    got = _C.rasterize_layers_cuda(*_dev(s, None if exist is None else s[exist]), L)
    torch.cuda.synchronize()
    _equal(got, want, (name, L, exist))
    assert want["cnt"].sum() > 0


def test_op_bit_equal_on_a_globally_sorted_list():
    """deep_sort: one tile whose list is longer than TILE_SORT_MAX (the plan's global radix sort), L = 17."""
    import tet_scenes
    s = ref.tet_case("deep_sort", *DEEP_SORT_SIZE)
    x = ref.tet_intersect("deep_sort", None, True, *DEEP_SORT_SIZE)
    assert (x["cand"] >= 0).sum(1).max() > tet_scenes.thresholds()["TILE_SORT_MAX"]
    got = _C.rasterize_layers_cuda(*_dev(s, None), 17)
    torch.cuda.synchronize()
    want = ref.select(x, 17)
    _equal(got, want, "deep_sort")
    assert (want["cnt"] == 17).any()


def test_analytic_rays_bit_equal_to_the_ray_tensor_path():
    from oracle import cpu as orc
    W, H, bidx = 88, 60, [1, 0]
    ts = scenes.tet_lattice(W, H, 5, seed=scenes.SEED_BASE + 82, num_cams=2).to("cuda")
    r_a = dm2.Renderer(ts.mv, ts.proj, W, H, "cuda", analytic_rays=True)
    cam = r_a.ray_cam.cpu().numpy()
    ro, rd = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), W, H)
    r_t = dm2.Renderer(ts.mv, ts.proj, W, H, "cuda")
    r_t.ray_o, r_t.ray_d = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    out = []
    for r in (r_a, r_t):
        v = ts.verts.clone().requires_grad_(True)
        res = r.rasterize(bidx, v, ts.faces, 6, faces_existence=ts.faces_existence)
        gb = torch.randn(res[2].shape, generator=torch.Generator().manual_seed(7)).cuda()
        gt = torch.randn(res[3].shape, generator=torch.Generator().manual_seed(8)).cuda()
        ((res[2] * gb).sum() + (res[3] * gt).sum()).backward()
        out.append([x.detach().cpu().numpy() for x in res] + [v.grad.cpu().numpy()])
    assert r_a.ray_o is None
    for k, (a, b) in enumerate(zip(out[0][:4], out[1][:4])):
        assert np.array_equal(_bits(a), _bits(b)), OUTS[k]
    assert (out[0][1] > 0).sum() > 1000
    assert rel_linf(out[0][4], out[1][4]) <= 2e-6


@pytest.mark.parametrize("n,seed", [(4, 70), (6, 71)])
def test_generate_is_a_prefix(n, seed):
    """GPU generate against GPU rasterize on lattices: generate's list is a prefix of rasterize's at every pixel, a near-tie
    along the ray (a shared edge or vertex) excused and counted."""
    W, H, L, bidx = 96, 72, 8, [1, 0]
    ts = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + seed, num_cams=2).to("cuda")
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda")
    gl, gc = lr.generate(bidx, ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, L)
    rl, rc, bary, t = lr.rasterize(bidx, ts.verts, ts.faces, L, faces_existence=ts.faces_existence)
    r = dict(layers=rl.cpu().numpy(), t=t.cpu().numpy())
    bad = ref.prefix_violations(gl.cpu().numpy(), gc.cpu().numpy(), r)
    ties = ref.near_ties(r)
    print(f"tet_lattice(n={n}): {int((bad & ties).sum())} of {bad.size} pixels excused (near-tie)")
    assert not (bad & ~ties).any()
    assert int((bad & ties).sum()) <= 0.001 * bad.size
    assert gc.sum() > 0.3 * rc.sum()


def _sheets(n_sheets, seed):
    """Fronto-parallel sheets (one large triangle each) at distinct depths in front of the default camera (the scene of
    test_gpu_layer_composite.py's test_agrees_with_renderer_at_temperature_zero)."""
    rng = np.random.RandomState(seed)
    verts, faces = [], []
    for s in range(n_sheets):
        z = 0.6 - 0.3 * s
        x0, y0 = rng.uniform(-1.2, -0.6, 2)
        x1, y1 = rng.uniform(0.6, 1.4, 2)
        b = len(verts)
        verts += [[x0, y0, z], [x1, y0, z], [x0, y1, z]] if s % 2 == 0 else [[x1, y1, z], [x0, y1, z], [x1, y0, z]]
        faces += [[b, b + 1, b + 2]]
    return torch.tensor(verts, dtype=torch.float32), torch.tensor(faces, dtype=torch.int32)


def test_composite_agrees_with_renderer_at_temperature_zero():
    """rasterize's ids are the brute-force depth-ordered code-0 hits; composited by LayeredRenderer.render they give
    Renderer(aa_temperature=0)'s colour and depth to 1e-6 and its gradients to GRAD_TOL."""
    import layer_composite_ref as lref
    W, H, S = 96, 80, 5
    L = S + 1
    mv, proj = scenes.camera(W, H)
    mv, proj = mv[None].cuda(), proj[None].cuda()
    verts, faces = _sheets(S, 5)
    P, F = verts.shape[0], faces.shape[0]
    g = np.random.RandomState(6)
    mat = dict(verts_color=g.uniform(0, 1, (P, 3)).astype(np.float32), faces_intense=g.uniform(0.5, 1.5, (1, F)).astype(np.float32),
               faces_opacity=np.random.RandomState(1).uniform(0.2, 0.8, F).astype(np.float32),
               background=np.array([0.1, 0.3, 0.7], np.float32))
    r = dm2.Renderer(mv, proj, W, H, "cuda")
    lr = dm2.LayeredRenderer(mv, proj, W, H, "cuda")
    ro, rd = r.ray_o[0].cpu().numpy(), r.ray_d[0].cpu().numpy()
    vn, fn = verts.numpy(), faces.numpy()
    ok, t, u, v = lref.ray_tri32(ro[:, :, None, :], rd[:, :, None, :], vn[fn[:, 0]], vn[fn[:, 1]], vn[fn[:, 2]])
    hit = ok & (lref.clamp_code32(u, v) == 0)
    order = np.argsort(np.where(hit, t, np.inf), axis=-1, kind="stable")[..., :L]
    brute = np.where(np.take_along_axis(hit, order, -1), order, -1).astype(np.int32)[None]
    brute = np.concatenate([brute, np.full(brute.shape[:3] + (L - brute.shape[3],), -1, np.int32)], -1)   # (S faces < L slots)
    layers, cnt, _, _ = lr.rasterize([0], verts.cuda(), faces.cuda(), L)
    assert int(cnt.max()) < L and (brute[..., 1] >= 0).sum() > 500
    assert np.array_equal(layers.cpu().numpy(), brute)
    wc = torch.randn((1, H, W, 3), generator=torch.Generator().manual_seed(3)).cuda()
    wd = torch.randn((1, H, W), generator=torch.Generator().manual_seed(4)).cuda()
    res = []
    for kind in ("renderer", "layers"):
        leaves = [torch.from_numpy(mat[k]).cuda().requires_grad_(True) for k in ("verts_color", "faces_opacity", "faces_intense")]
        bg = torch.from_numpy(mat["background"]).cuda()
        if kind == "renderer":
            color, depth = r([0], torch.zeros((1, 2), dtype=torch.int64, device="cuda"), W, H, verts.cuda(), faces.cuda(),
                             leaves[0], leaves[1], leaves[2], bg, aa_temperature=0.0)
        else:
            color, depth = lr.render([0], layers, verts.cuda(), faces.cuda(), leaves[0], leaves[1], leaves[2], bg)
        ((color * wc).sum() + (depth * wd).sum()).backward()
        res.append((color.detach().cpu().numpy(), depth.detach().cpu().numpy(), [x.grad.cpu().numpy() for x in leaves]))
    (c0, d0, g0), (c1, d1, g1) = res
    assert np.abs(c0 - c1).max() <= 1e-6 and np.abs(d0 - d1).max() <= 1e-6
    for a, b in zip(g1, g0):
        assert np.abs(b).max() > 0 and rel_linf(a, b) <= GRAD_TOL


@pytest.mark.parametrize("name", ["soup", "lattice"])
@pytest.mark.parametrize("L", [2, 4, 16, 40])
def test_gradients_against_float64(name, L):
    s = _scene(name)
    args = _dev(s, s["fe"])
    layers, cnt, bary, t = _C.rasterize_layers_cuda(*args, L)
    gen = torch.Generator().manual_seed(L)
    gb = torch.randn(bary.shape, generator=gen)
    gt = torch.randn(t.shape, generator=gen)
    W, H, verts, faces, _, _, _, ro, rd = args
    for g_b, g_t in ((gb, gt), (gb, None), (None, gt)):
        got = _C.rasterize_layers_backward_cuda(layers, verts, faces, ro, rd, None if g_b is None else g_b.cuda(),
                                                None if g_t is None else g_t.cuda()).cpu().numpy()
        want = ref.grads64(s["verts"], s["faces"], layers.cpu(), s["ray_o"], s["ray_d"], g_b, g_t)
        assert np.isfinite(got).all() and np.abs(want).max() > 0
        assert rel_linf(got, want) <= GRAD_TOL, (name, L, g_b is None, g_t is None, rel_linf(got, want))
    if L == 40 and name == "soup":
        assert int(cnt.max()) > 16                                             # (hits from the second pass)


@pytest.mark.parametrize("name", ["aligned", "flat", "duplicates", "inside"])
@pytest.mark.parametrize("L", [4, 17])
def test_gradients_against_float64_on_tet_scenes(name, L):
    """The backward on the kernel's own lists of the tet scenes: hits on edges and vertices, faces seen at grazing angles down
    to the hit rule's |cos| > 5e-4 (aligned), faces listed twice (duplicates), a camera inside the mesh."""
    s = ref.tet_case(name)
    args = _dev(s, s["fe"])
    layers, cnt, bary, t = _C.rasterize_layers_cuda(*args, L)
    gen = torch.Generator().manual_seed(L)
    gb = torch.randn(bary.shape, generator=gen)
    gt = torch.randn(t.shape, generator=gen)
    W, H, verts, faces, _, _, _, ro, rd = args
    for g_b, g_t in ((gb, gt), (gb, None), (None, gt)):
        got = _C.rasterize_layers_backward_cuda(layers, verts, faces, ro, rd, None if g_b is None else g_b.cuda(),
                                                None if g_t is None else g_t.cuda()).cpu().numpy()
        want = ref.grads64(s["verts"], s["faces"], layers.cpu(), s["ray_o"], s["ray_d"], g_b, g_t)
        assert np.isfinite(got).all() and np.isfinite(want).all() and np.abs(want).max() > 0
        print(name, L, g_b is None, g_t is None, rel_linf(got, want))
        assert rel_linf(got, want) <= GRAD_TOL, (name, L, g_b is None, g_t is None, rel_linf(got, want))
    if L == 17 and name != "inside":
        assert int(cnt.max()) > 16                                             # (hits from the second pass)


@pytest.mark.parametrize("name", ["overflow_L4", "overflow_L12", "nearly_full_L4"])
def test_backward_table_overflow_route(name):
    """k_rasterize_bwd where lc_slot finds no slot: a hit's nine components go to global memory as per-hit float casts
    instead of into the fp64 LDS sum.  The lists, triangles and orthographic rays of the compositor's crowded scenes
    (layer_composite_ref.CROWDED; the backward takes any lists, it needs no forward), a few ids out of range among them:
    every 16 x 16 tile lists more distinct faces than the table holds, or nearly as many."""
    import layer_composite_ref as lref
    sc, kind = lref.crowded_case(name)
    F = sc["faces"].shape[0]
    rl = sc["render_layers"].copy()
    pick = np.random.RandomState(9).choice(rl.size, 600, replace=False)
    rl.reshape(-1)[pick] = np.array([-1, F, F + 7], np.int32)[np.arange(600) % 3]
    listed = (rl >= 0) & (rl < F)                          # (this kernel's table is keyed by every listed id in range)
    lo, hi = lref.distinct_blended_per_tile(dict(blend=listed, fs=rl))
    print(f"rasterize backward {name}: {lo}..{hi} distinct listed faces per tile, table of {table_capacity()} slots")
    lref.check_crowded(kind, lo, hi, table_capacity())
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    layers, verts, faces, ro, rd = c(rl), c(sc["verts"]), c(sc["faces"]), c(sc["ray_o"]), c(sc["ray_d"])
    gen = torch.Generator().manual_seed(10)
    gb = torch.randn(rl.shape + (3,), generator=gen)
    gt = torch.randn(rl.shape, generator=gen)
    for g_b, g_t in ((gb, gt), (gb, None), (None, gt)):
        got = _C.rasterize_layers_backward_cuda(layers, verts, faces, ro, rd, None if g_b is None else g_b.cuda(),
                                                None if g_t is None else g_t.cuda()).cpu().numpy()
        want = ref.grads64(sc["verts"], sc["faces"], rl, sc["ray_o"], sc["ray_d"], g_b, g_t)
        assert np.isfinite(got).all() and np.abs(want).max() > 0
        assert (np.abs(want).max(-1) > 0).sum() > 0.9 * want.shape[0]          # (nearly every vertex has a gradient to lose)
        assert rel_linf(got, want) <= GRAD_TOL, (name, g_b is None, g_t is None, rel_linf(got, want))


def test_module_path():
    """Both host preps and analytic rays: each run equals the restatement of the very inputs its op got; no graph under
    no_grad; a loss on interpolated colour reaches verts; with bary and t outside the loss no backward kernel runs."""
    W, H, bidx, L = 80, 64, [0, 1], 5
    ts = scenes.tet_lattice(W, H, 4, seed=scenes.SEED_BASE + 83, num_cams=2).to("cuda")
    seen = []
    real = _C.rasterize_layers_cuda

    def spy(*a):
        out = real(*a)
        seen.append(([x.detach().cpu().numpy() if torch.is_tensor(x) else x for x in a], out))
        return out
    _C.rasterize_layers_cuda = spy
    try:
        for kw in (dict(fused_prep=False), dict(fused_prep=True), dict(analytic_rays=True)):
            r = dm2.Renderer(ts.mv, ts.proj, W, H, "cuda", **kw)
            r.rasterize(bidx, ts.verts, ts.faces, L, faces_existence=ts.faces_existence)
            a, out = seen[-1]
            if kw.get("analytic_rays"):
                from oracle import cpu as orc
                cam = r.ray_cam.cpu().numpy()
                a[7], a[8] = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), W, H)
            want = ref.rasterize32(*a[:9], L)
            _equal(out, want, kw)
    finally:
        _C.rasterize_layers_cuda = real
    r = dm2.Renderer(ts.mv, ts.proj, W, H, "cuda")
    verts = ts.verts.clone().requires_grad_(True)
    with torch.no_grad():
        out = r.rasterize(bidx, verts, ts.faces, L)
    assert all(x.grad_fn is None for x in out)
    colors = torch.rand((verts.shape[0], 3), generator=torch.Generator().manual_seed(2)).cuda()
    ids, cnt, bary, t = r.rasterize(bidx, verts, ts.faces, L)
    assert ids.grad_fn is None and bary.grad_fn is not None
    img = (bary[..., None] * colors[ts.faces.long()[ids.clamp(min=0).long()]]).sum(-2)       # (B,H,W,L,3); -1 slots weigh -1
    img = torch.where((ids >= 0)[..., None], img, torch.zeros_like(img))
    img.sum().backward()
    assert verts.grad is not None and torch.isfinite(verts.grad).all() and verts.grad.abs().max() > 0
    calls = []
    real_b = _C.rasterize_layers_backward_cuda
    _C.rasterize_layers_backward_cuda = lambda *a: calls.append(1) or real_b(*a)
    try:
        v2 = ts.verts.clone().requires_grad_(True)
        ids, cnt, bary, t = r.rasterize(bidx, v2, ts.faces, L)
        (v2.sum() + cnt.float().sum() * 0).backward()
        assert not calls
        ids, cnt, bary, t = r.rasterize(bidx, v2, ts.faces, L)
        t.sum().backward()
        assert len(calls) == 1
    finally:
        _C.rasterize_layers_backward_cuda = real_b


def test_module_path_on_aligned():
    """LayeredRenderer.rasterize on ``aligned`` (rays in face planes: the hit rule decides) with both host preps and with
    analytic rays: each run equals the restatement of the very inputs its op got."""
    import tet_scenes
    ts, _ = tet_scenes.case("aligned")
    W, H, bidx, L = ts.width, ts.height, [0, 1], 5
    ts = ts.to("cuda")
    seen = []
    real = _C.rasterize_layers_cuda

    def spy(*a):
        out = real(*a)
        seen.append(([x.detach().cpu().numpy() if torch.is_tensor(x) else x for x in a], out))
        return out
    _C.rasterize_layers_cuda = spy
    try:
        for kw in (dict(fused_prep=False), dict(fused_prep=True), dict(analytic_rays=True)):
            lr = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda", **kw)
            lr.rasterize(bidx, ts.verts, ts.faces, L, faces_existence=ts.faces_existence)
            a, out = seen[-1]
            if kw.get("analytic_rays"):
                from oracle import cpu as orc
                cam = lr.ray_cam.cpu().numpy()
                a[7], a[8] = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), W, H)
            x_old, x = (ref.intersect(*a[:9], rule=rule) for rule in (False, True))
            _equal(out, ref.select(x, L), kw)
            removed = ref.rule_removed(x_old, x)
            print(f"aligned, {kw}: the hit rule removes {removed[0]} hits at {removed[1]} pixels")
            assert removed[0] > 0, kw
    finally:
        _C.rasterize_layers_cuda = real
