"""LayeredRenderer.render / dm2_layers_composite on the GPU against the contract's restatement (tests/layer_composite_ref.py):
forward bit-equal to the float32 pass, gradients within GRAD_TOL of the float64 pass; agreement with Renderer at
aa_temperature 0 where both must agree; the face table's overflow route and a nearly full table on crowded scenes; layer lists
at unaligned addresses; analytic rays; the module path with both host preps; full size."""
import numpy as np
import pytest
import torch

import layer_composite_ref as ref
from util import GRAD_TOL, rel_linf, scenes, table_capacity

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

GRADS = ("verts_color", "faces_opacity", "verts_ndc", "faces_intense")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.int32)


def _check_op(inp, seed=0):
    """Run the op (forward + backward) on `inp` (numpy / torch inputs of composite_layers_cuda) and hold it to the restatement."""
    dev = "cuda"
    t = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(dev) for k, v in inp.items()}
    args = [t[k] for k in ("render_layers", "verts", "faces", "verts_color", "faces_opacity", "faces_intense", "verts_ndc",
                           "background", "ray_o", "ray_d")]
    color, depth, final_T, n_contrib = _C.composite_layers_cuda(*args)
    gen = torch.Generator().manual_seed(seed)
    gc = torch.randn(color.shape, generator=gen)
    gd = torch.randn(depth.shape, generator=gen)
    grads = _C.composite_layers_backward_cuda(*args, n_contrib, gc.to(dev), gd.to(dev))
    torch.cuda.synchronize()
    fwd = ref.forward32(*[a.cpu() for a in args])
    for name, got in (("color", color), ("depth_raw", depth), ("final_T", final_T), ("n_contrib", n_contrib)):
        g = got.cpu().numpy()
        assert np.array_equal(_bits(g), _bits(fwd[name])), (name, int((_bits(g) != _bits(fwd[name])).sum()))
    want = ref.grads64(fwd, args[2].cpu(), args[3].cpu(), args[4].cpu(), args[5].cpu(), args[6].cpu(), args[7].cpu(),
                       gc.double(), gd.double())
    for name, got in zip(GRADS, grads):
        g = got.cpu().numpy()
        assert np.isfinite(g).all(), name
        assert rel_linf(g, want[name]) <= GRAD_TOL, (name, rel_linf(g, want[name]))
    return fwd, want


def _material(P, F, B, seed):
    g = np.random.RandomState(seed)
    return dict(verts_color=g.uniform(0, 1, (P, 3)).astype(np.float32), faces_opacity=g.uniform(0.05, 0.95, F).astype(np.float32),
                faces_intense=g.uniform(0.5, 1.5, (B, F)).astype(np.float32), background=np.array([0.1, 0.3, 0.7], np.float32))


def _generated(W, H, n, bidx, L, seed, num_cams=2, analytic=False):
    ts = scenes.tet_lattice(W, H, n, seed=seed, num_cams=num_cams).to("cuda")
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda", analytic_rays=analytic)
    layers, _ = lr.generate(bidx, ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, L)
    return ts, lr, layers


@pytest.mark.parametrize("L", [1, 4, 8])
def test_generate_layers_small(L):
    bidx = [1, 0]
    ts, lr, layers = _generated(200, 120, 6, bidx, L, scenes.SEED_BASE + 60)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    ndc, _ = lr.compute_verts_ndc_image(ts.verts, ts.mv[bidx], ts.proj[bidx])
    inp = dict(render_layers=layers, verts=ts.verts, faces=ts.faces, verts_ndc=ndc.contiguous(),
               ray_o=lr.ray_o[bidx].contiguous(), ray_d=lr.ray_d[bidx].contiguous(), **_material(P, F, 2, L))
    fwd, want = _check_op(inp, seed=L)
    assert fwd["blend"].sum() > 1000 and np.abs(want["faces_opacity"]).max() > 0


@pytest.mark.parametrize("L", [5, 8, 12])
def test_hand_built_lists(L):
    """Holes (-1 mid-list), ids >= F, negative ids, the same face repeated in a pixel's list, opacities of exactly 0 and 1;
    L = 12 runs the backward's path for lists longer than its register chunk."""
    sc = ref.ortho_scene(B=2, H=37, W=45, L=L, F=11, seed=L)
    rl = sc["render_layers"]
    rl[:, ::3, :, 1] = rl[:, ::3, :, 0]                                       # repeats
    sc["faces_opacity"][[2, 5]] = [0.0, 1.0]
    fwd, want = _check_op(sc, seed=100 + L)
    assert ((rl < 0) | (rl >= 11)).any() and fwd["blend"].sum() > 500
    assert (fwd["final_T"] == 0.0).any()                                      # an opacity-1 face ended some lists
    # every kind of layer occurs in the blends
    f_bl = np.where(fwd["blend"], fwd["fs"], -1)
    assert (f_bl == 5).any() and (f_bl == 2).any()


def crowded(name, what):
    """A crowded case of the restatement (layer_composite_ref.CROWDED) with the condition it is there for asserted on the
    restatement's own blends, and the range printed."""
    sc, kind = ref.crowded_case(name)
    fwd = ref.forward32(**sc)
    lo, hi = ref.distinct_blended_per_tile(fwd)
    print(f"{what} {name}: {lo}..{hi} distinct blended faces per tile, table of {table_capacity()} slots")
    ref.check_crowded(kind, lo, hi, table_capacity())
    return sc


@pytest.mark.parametrize("name", list(ref.CROWDED))
def test_table_overflow_route(name):
    """k_layer_composite_bwd<false> where lc_slot finds no slot: every face covers the frame, so a 16 x 16 tile blends more
    distinct faces than the table holds (overflow: most hits add their 14 components straight to global memory) or nearly as
    many (nearly full: probe chains fail for a few faces while slots remain free, both routes in one tile).  B = 2: the
    view offsets of dndc and dintense count.  Opacities of exactly 0 and 1 and a face twice in a pixel's list, as in
    test_hand_built_lists."""
    sc = crowded(name, "composite")
    fwd, want = _check_op(sc, seed=7)
    f_bl = np.where(fwd["blend"], fwd["fs"], -1)
    assert (fwd["final_T"] == 0.0).any() and (sc["faces_opacity"][f_bl[f_bl >= 0]] == 0.0).any()
    assert ((f_bl[..., 0] == f_bl[..., 1]) & (f_bl[..., 0] >= 0)).any()
    assert all(np.abs(want[k]).max() > 0 for k in GRADS)
    assert (np.abs(want["faces_intense"][1]) > 0).sum() > 0.5 * sc["faces"].shape[0]          # (the second view's rows too)


@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("skip", [1, 2], ids=["4_bytes", "8_bytes"])
def test_unaligned_layers_give_the_same_bits(L, skip):
    """render_layers as a contiguous view that starts 4 or 8 bytes into its storage: launch_layer_composite reads the ids one
    at a time or as 8-byte pairs instead of 16-byte vectors.  Same forward bits as the aligned call, gradients within
    GRAD_TOL of float64, and the same once more with face weights."""
    from face_weights_ref import layered_face_weights64
    from test_gpu_face_weights import check_weights
    sc = ref.ortho_scene(B=2, H=37, W=45, L=L, F=11, seed=20 + L)
    sc["render_layers"][:, ::3, :, 1] = sc["render_layers"][:, ::3, :, 0]
    sc["faces_opacity"][[2, 5]] = [0.0, 1.0]
    aligned = torch.from_numpy(sc["render_layers"]).cuda()
    store = torch.empty(aligned.numel() + 4, dtype=torch.int32, device="cuda")
    v = store[skip:skip + aligned.numel()].view(aligned.shape)
    v.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0
    assert v.data_ptr() % 16 in (4, 8) and v.data_ptr() % 16 == 4 * skip and v.is_contiguous()
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).cuda() for k, x in sc.items()}
    names = ("verts", "faces", "verts_color", "faces_opacity", "faces_intense", "verts_ndc", "background", "ray_o", "ray_d")
    rest = [t[k] for k in names]
    want = _C.composite_layers_cuda(aligned, *rest)
    got = _C.composite_layers_cuda(v, *rest)
    with _C.face_weights_output(True):
        want_w = _C.composite_layers_cuda(aligned, *rest)
        got_w = _C.composite_layers_cuda(v, *rest)
    torch.cuda.synchronize()
    assert len(got) == 4 and len(got_w) == 5
    for i in range(4):
        assert torch.equal(got[i], want[i]) and torch.equal(got_w[i], want[i]) and torch.equal(want_w[i], want[i]), i
    fwd, _ = _check_op(dict(sc, render_layers=v), seed=30 + L)                 # (forward bits and the four gradients, from v)
    assert fwd["blend"].sum() > 500
    check_weights(got_w[4], layered_face_weights64(fwd, sc["faces_opacity"], sc["faces"].shape[0]), min_nonzero=3)


def _sheets(W, H, n_sheets, seed):
    """Fronto-parallel sheets (one large triangle each) at distinct depths in front of the default camera."""
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


def _spy(name, store):
    real = getattr(_C, name)

    def f(*a):
        out = real(*a)
        store[name] = out
        return out
    return real, f


def test_agrees_with_renderer_at_temperature_zero():
    """Layers = each pixel's code-0 hits in depth order: the compositor and Renderer(aa_temperature=0) must agree."""
    W, H, S = 96, 80, 5
    mv, proj = scenes.camera(W, H)
    mv, proj = mv[None].cuda(), proj[None].cuda()
    verts, faces = _sheets(W, H, S, 5)
    P, F = verts.shape[0], faces.shape[0]
    mat = _material(P, F, 1, 6)
    mat["faces_opacity"] = np.random.RandomState(1).uniform(0.2, 0.8, F).astype(np.float32)
    r = dm2.Renderer(mv, proj, W, H, "cuda")
    lr = dm2.LayeredRenderer(mv, proj, W, H, "cuda")
    # per-pixel code-0 hits sorted by ray distance
    ro, rd = r.ray_o[0].cpu().numpy(), r.ray_d[0].cpu().numpy()
    vn, fn = verts.numpy(), faces.numpy()
    ok, t, u, v = ref.ray_tri32(ro[:, :, None, :], rd[:, :, None, :], vn[fn[:, 0]], vn[fn[:, 1]], vn[fn[:, 2]])
    hit = ok & (ref.clamp_code32(u, v) == 0)
    key = np.where(hit, t, np.inf)
    order = np.argsort(key, axis=-1, kind="stable")[..., :S]
    layers = np.where(np.take_along_axis(hit, order, -1), order, -1).astype(np.int32)[None]
    assert (layers[..., 1] >= 0).sum() > 500
    g = torch.Generator().manual_seed(3)
    wc, wd = torch.randn((1, H, W, 3), generator=g).cuda(), torch.randn((1, H, W), generator=g).cuda()
    res = []
    store = {}
    reals = [_spy(n, store) for n in ("render_backward_cuda", "composite_layers_backward_cuda")]
    for n, (_, f) in zip(("render_backward_cuda", "composite_layers_backward_cuda"), reals):
        setattr(_C, n, f)
    try:
        for kind in ("renderer", "layers"):
            leaves = [verts.cuda().requires_grad_(True)] + [torch.from_numpy(mat[k]).cuda().requires_grad_(True)
                                                            for k in ("verts_color", "faces_opacity", "faces_intense")]
            if kind == "renderer":
                color, depth = r([0], torch.zeros((1, 2), dtype=torch.int64, device="cuda"), W, H, leaves[0], faces.cuda(),
                                 leaves[1], leaves[2], leaves[3], torch.from_numpy(mat["background"]).cuda(), aa_temperature=0.0)
            else:
                color, depth = lr.render([0], torch.from_numpy(layers).cuda(), leaves[0], faces.cuda(), leaves[1], leaves[2],
                                         leaves[3], torch.from_numpy(mat["background"]).cuda())
            ((color * wc).sum() + (depth * wd).sum()).backward()
            torch.cuda.synchronize()
            res.append((color.detach().cpu().numpy(), depth.detach().cpu().numpy(), [x.grad.cpu().numpy() for x in leaves[1:]]))
    finally:
        for n, (real, _) in zip(("render_backward_cuda", "composite_layers_backward_cuda"), reals):
            setattr(_C, n, real)
    (c0, d0, g0), (c1, d1, g1) = res
    bit_equal = np.array_equal(c0, c1) and np.array_equal(d0, d1)
    print(f"compositor vs Renderer(aa_temperature=0): colour/depth bit-equal = {bit_equal}, "
          f"max |dc| = {np.abs(c0 - c1).max():.3g}, max |dd| = {np.abs(d0 - d1).max():.3g}")
    assert np.abs(c0 - c1).max() <= 1e-6 and np.abs(d0 - d1).max() <= 1e-6
    for a, b in zip(g1, g0):
        assert rel_linf(a, b) <= GRAD_TOL
    ndc_r = store["render_backward_cuda"][3].cpu().numpy()
    ndc_l = store["composite_layers_backward_cuda"][2].cpu().numpy()
    assert np.abs(ndc_r).max() > 0 and rel_linf(ndc_l[..., 2], ndc_r[..., 2]) <= GRAD_TOL
    assert np.abs(g0[1]).max() > 0


def test_analytic_rays_bit_equal_to_the_ray_tensor_path():
    from oracle import cpu as orc
    W, H, bidx = 160, 96, [1, 0]
    ts, lr_a, layers = _generated(W, H, 5, bidx, 4, scenes.SEED_BASE + 61, analytic=True)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    mat = {k: torch.from_numpy(v).cuda() for k, v in _material(P, F, 2, 9).items()}
    cam = lr_a.ray_cam.cpu().numpy()
    ro, rd = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), W, H)
    lr_t = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda")
    lr_t.ray_o, lr_t.ray_d = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    g = torch.Generator().manual_seed(4)
    wc, wd = torch.randn((2, H, W, 3), generator=g).cuda(), torch.randn((2, H, W), generator=g).cuda()
    out = []
    for lr in (lr_a, lr_t):
        leaves = [mat[k].clone().requires_grad_(True) for k in ("verts_color", "faces_opacity", "faces_intense")]
        color, depth = lr.render(bidx, layers, ts.verts, ts.faces, leaves[0], leaves[1], leaves[2], mat["background"])
        ((color * wc).sum() + (depth * wd).sum()).backward()
        out.append((color.detach().cpu().numpy(), depth.detach().cpu().numpy(), [x.grad.cpu().numpy() for x in leaves]))
    (ca, da, ga), (ct, dt, gt) = out
    assert lr_a.ray_o is None
    assert np.array_equal(_bits(ca), _bits(ct)) and np.array_equal(_bits(da), _bits(dt))
    assert (ca != mat["background"].cpu().numpy()).any()
    for a, b in zip(ga, gt):
        assert rel_linf(a, b) <= 2e-6


def test_module_path_both_preps():
    W, H, bidx = 128, 96, [0, 1]
    ts, lr, layers = _generated(W, H, 5, bidx, 4, scenes.SEED_BASE + 62)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    mat = {k: torch.from_numpy(v).cuda() for k, v in _material(P, F, 2, 10).items()}
    g = torch.Generator().manual_seed(5)
    wc, wd = torch.randn((2, H, W, 3), generator=g).cuda(), torch.randn((2, H, W), generator=g).cuda()
    res = []
    for fused in (False, True):
        m = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, "cuda", fused_prep=fused)
        leaves = [ts.verts.clone().requires_grad_(True)] + [mat[k].clone().requires_grad_(True)
                                                           for k in ("verts_color", "faces_opacity", "faces_intense")]
        color, depth = m.render(bidx, layers, leaves[0], ts.faces, leaves[1], leaves[2], leaves[3], mat["background"])
        loss = (color * wc).sum() + (depth * wd).sum()
        loss.backward()
        torch.cuda.synchronize()
        grads = [x.grad for x in leaves]
        assert all(gr is not None and torch.isfinite(gr).all() and gr.abs().max() > 0 for gr in grads), fused
        res.append((color.detach().cpu().numpy(), depth.detach().cpu().numpy(), [gr.cpu().numpy() for gr in grads]))
    (c0, d0, g0), (c1, d1, g1) = res
    assert np.abs(c0 - c1).max() <= 1e-4 and np.abs(d0 - d1).max() <= 1e-4
    for a, b in zip(g0, g1):
        assert rel_linf(b, a) <= 1e-3


def test_full_size_cfg3():
    """SURVEY.md 8(d) cfg 3: 1024^2, tet_lattice(n=25), L = 4 from generate, B = 1."""
    W = H = 1024
    ts, lr, layers = _generated(W, H, 25, [0], 4, scenes.SEED_BASE + 3, num_cams=1)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    ndc, _ = lr.compute_verts_ndc_image(ts.verts, ts.mv[[0]], ts.proj[[0]])
    inp = dict(render_layers=layers, verts=ts.verts, faces=ts.faces, verts_ndc=ndc.contiguous(),
               ray_o=lr.ray_o[[0]].contiguous(), ray_d=lr.ray_d[[0]].contiguous(), **_material(P, F, 1, 3))
    fwd, _ = _check_op(inp, seed=33)
    assert fwd["blend"].sum() > 100000
