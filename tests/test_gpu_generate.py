"""LayeredRenderer.generate (k_first_intersect, k_pack_tets, k_tet_walk_rec / k_tet_walk after dm2_layers_plan / dm2_layers_run)
held to the CPU oracle where tet walks break: the scenes of tests/tet_scenes.py (rays through vertices, along edges and in face
planes; deleted tets and orphan faces; cameras inside the mesh; inverted tets and zero-area faces; duplicated faces; tile
lists of many staging chunks and beyond the plan's per-tile sort), every existence table, both walks, odd image sizes.
tests/test_generate_cpu.py shows on the oracle's output that each scene is what it claims.  Also: the op's paths against each
other bit for bit, a float64 brute force on the GPU's output, a fixed seeded part of tests/fuzz_layers.py's sweep, the layer
compositor on generate's odd outputs, and the argument checks.  Every case runs once; nothing here is meant to fault."""
import numpy as np
import pytest
import torch

import fuzz_layers
import generate_ref as G
import layer_composite_ref as lref
import tet_scenes as S
from test_generate_cpu import BRUTE, L_ALL, brute_case
from util import _C, spy_library

pytestmark = pytest.mark.gpu

LS = (0, 1, 2, 4, 7)
WALKS = (("records", 0), ("legacy", _C.DM2_FLAG_LEGACY_KERNELS))
SCENES = tuple(S.CASES)


def _bidx(ts, B):
    """B = 1: camera 0; B = 3: the last camera twice around camera 0 (a repeated index)."""
    last = ts.mv.shape[0] - 1
    return [0] if B == 1 else [last, 0, last]


def _generate(lr, scd, bidx, L, flags, existence=None):
    """generate under ``flags`` -> layers, cnt, first_face, first_tet (numpy), num_rendered."""
    ex = scd.faces_existence if existence is None else existence
    old = _C.set_flags(flags)
    try:
        layers, cnt = lr.generate(bidx, scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, ex, L)
    finally:
        _C.set_flags(old)
    B, H, W = cnt.shape
    R, face_buf, bin_buf, img_buf = _C.generate_render_layers_cuda.last_debug
    N, Tn = B * H * W, _C._tiles(B, W, H)
    ff = _C.debug_fetch(5, N, Tn, R, img_buf, torch.int32, N).cpu().numpy().reshape(B, H, W)
    ft = _C.debug_fetch(6, N, Tn, R, img_buf, torch.int32, N).cpu().numpy().reshape(B, H, W)
    assert layers.dtype == torch.int32 and cnt.dtype == torch.int32 and tuple(layers.shape) == (B, H, W, L)
    return layers.cpu().numpy(), cnt.cpu().numpy(), ff, ft, R


def _check(ts, bidx, Ls, existence=None, what="", deepest=True):
    """The op on scene ``ts`` for every L of ``Ls`` (and one above the deepest walk), both walks: first_face, first_tet,
    render_layers_cnt and render_layers equal the oracle's; slots at and beyond the count are -1."""
    scd = ts.to("cuda")
    lr = S.renderer(ts, "cuda")
    inp = G.inputs(lr, scd.verts, bidx)
    ex_np = None if existence is None else np.asarray(existence, np.int32)
    ex_dev = None if existence is None else torch.from_numpy(ex_np).cuda()
    Ls = tuple(Ls)
    if deepest:
        top = int(G.oracle(ts, inp, L_ALL, existence=ex_np)["cnt"].max()) + 1
        assert top <= L_ALL
        Ls += (top,)
    for L in Ls:
        o = G.oracle(ts, inp, L, existence=ex_np)
        for walk, flags in WALKS:
            layers, cnt, ff, ft, R = _generate(lr, scd, bidx, L, flags, ex_dev)
            tag = (what, "L", L, walk)
            assert R == o["bn"].num_rendered, tag
            assert np.array_equal(ff, o["ff"]), tag + ("first_face", int((ff != o["ff"]).sum()))
            assert np.array_equal(ft, o["ft"]), tag + ("first_tet", int((ft != o["ft"]).sum()))
            assert np.array_equal(cnt, o["cnt"]), tag + ("cnt", int((cnt != o["cnt"]).sum()))
            assert np.array_equal(layers, o["layers"]), tag + ("layers", int((layers != o["layers"]).any(-1).sum()))
            assert (layers[np.arange(L)[None, None, None] >= cnt[..., None]] == -1).all(), tag
    return o


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", SCENES)
def test_exact(name, B):
    ts, _ = S.case(name)
    o = _check(ts, _bidx(ts, B), LS, what=name)
    assert (o["cnt"] > 0).mean() > 0.1


@pytest.mark.parametrize("size", [(1, 1), (17, 33)])
@pytest.mark.parametrize("name", [n for n in SCENES if n not in S.FIXED_SIZE])
def test_exact_odd_sizes(name, size):
    ts, _ = S.case(name, *size)
    assert (ts.width, ts.height) == size
    _check(ts, _bidx(ts, 3), (0, 2), what=(name, size))


@pytest.mark.parametrize("table", ["zeros", "ones", "odd"])
@pytest.mark.parametrize("name", [n for n in SCENES if n not in S.FIXED_SIZE])
def test_exact_existence_tables(name, table):
    ts, _ = S.case(name)
    tab = S.existence_tables(ts.faces.shape[0], 11)[table]
    o = _check(ts, _bidx(ts, 1), (4,), existence=tab, what=(name, table), deepest=table != "zeros")
    assert (o["cnt"] > 0).any() == (table != "zeros")


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int64])
def test_existence_dtypes_through_the_module(dtype):
    """The module converts the flags to int32 (bool: 0 / 1; uint8 wraps -1 to 255 and INT_MIN to 0; int64 keeps the values)."""
    ts, _ = S.case("holes")
    tab = torch.from_numpy(S.existence_tables(ts.faces.shape[0], 12)["odd"])
    given = (tab != 0) if dtype == torch.bool else tab.to(dtype)
    scd = ts.to("cuda")
    lr = S.renderer(ts, "cuda")
    bidx = [1, 0]
    inp = G.inputs(lr, scd.verts, bidx)
    o = G.oracle(ts, inp, 5, existence=given.to(torch.int32).numpy())
    for walk, flags in WALKS:
        layers, cnt, ff, ft, _ = _generate(lr, scd, bidx, 5, flags, given.cuda())
        assert np.array_equal(layers, o["layers"]) and np.array_equal(cnt, o["cnt"]), (dtype, walk)
    assert (o["cnt"] > 0).mean() > 0.2


@pytest.mark.parametrize("name", ["aligned", "holes", "inside"])
def test_paths_agree_bit_for_bit(name):
    """fused_prep True against False, and analytic_rays=True against the ray-tensor path fed the same closed-form rays."""
    from oracle import cpu as orc
    ts, _ = S.case(name)
    scd = ts.to("cuda")
    bidx, L = _bidx(ts, 3), 6
    W, H = ts.width, ts.height

    def run(lr, flags):
        old = _C.set_flags(flags)
        try:
            out = lr.generate(bidx, scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, scd.faces_existence, L)
        finally:
            _C.set_flags(old)
        return out

    for walk, flags in WALKS:
        a = run(S.renderer(ts, "cuda", fused_prep=False), flags)
        b = run(S.renderer(ts, "cuda", fused_prep=True), flags)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (name, walk, "fused_prep")
        la = S.renderer(ts, "cuda", analytic_rays=True)
        cam = la.ray_cam.cpu().numpy()
        ro, rd = orc.analytic_rays_from_inverse(cam[:, :16].reshape(-1, 4, 4), cam[:, 16:].reshape(-1, 4, 4), W, H)
        lt = S.renderer(ts, "cuda")
        lt.ray_o, lt.ray_d = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
        c, d = run(la, flags), run(lt, flags)
        assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]), (name, walk, "analytic_rays")
        assert (c[1] > 0).float().mean() > 0.1


@pytest.mark.parametrize("n,seed,table", [c for c in BRUTE if c[2] != "ones"])
def test_gpu_output_against_float64_brute_force(n, seed, table):
    """tests/test_generate_cpu.py's brute-force check, on what the kernels return (the GPU's own projection and rays)."""
    ts, _, tab = brute_case(n, seed, table)
    scd = ts.to("cuda")
    lr = S.renderer(ts, "cuda")
    bidx = [1, 0]
    inp = G.inputs(lr, scd.verts, bidx)
    br8 = G.brute64(ts.verts, ts.faces, tab, inp["ro"], inp["rd"], 8, hull=S.hull_faces(ts))
    ex = torch.from_numpy(np.asarray(tab, np.int32)).cuda()
    for L in (8, 2):
        for walk, flags in WALKS:
            layers, cnt, _, _, _ = _generate(lr, scd, bidx, L, flags, ex)
            G.check_brute(layers, cnt, G.cut(br8, L), f"HIP ({walk}), tet_lattice(n={n}), existence {table}, L={L}")


# ---- the sweep as a gate -----------------------------------------------------------------------------------------------------
GATE = fuzz_layers.gate()


@pytest.mark.parametrize("seed,idx", GATE)
def test_sweep_gate(seed, idx):
    p = fuzz_layers.draw(seed, idx)
    ok, hit = fuzz_layers.run_case(p)
    assert ok, p


def test_sweep_gate_covers_every_axis():
    ps = [fuzz_layers.draw(*c) for c in GATE]
    for key, values in (("jitter", fuzz_layers.JITTERS), ("existence", fuzz_layers.EXISTENCE), ("cams", fuzz_layers.CAMS),
                        ("L", fuzz_layers.LAYERS), ("holes", fuzz_layers.HOLES), ("values", fuzz_layers.EXISTENCE_VALUES)):
        assert {p[key] for p in ps} == set(values), key
    assert any(p["jitter"] == 0.0 and p["existence"] == 1.0 and p["holes"] == 0.0 for p in ps)
    assert any(p["jitter"] == 0.0 and p["existence"] == 1.0 and p["holes"] > 0.0 for p in ps)
    assert len(set(GATE)) == len(GATE)
    # the scenes are what was drawn
    p = next(p for p in ps if p["holes"] > 0 and p["values"] == "odd" and p["n"] >= 2)
    sc = fuzz_layers.scene(p)
    assert (sc.face_tets.numpy() < 0).all(1).any() and set(np.unique(sc.faces_existence.numpy())) - {0, 1}


# ---- consumers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["holes", "duplicates"])
def test_render_composites_generated_layers(name):
    """generate's layers on scenes with orphans, cavities and duplicated faces, fed to LayeredRenderer.render: colour bit-equal
    to layer_composite_ref's float32 pass, depth and alpha within test_gpu_layer_composite.py's 1e-6."""
    ts, _ = S.case(name)
    scd = ts.to("cuda")
    lr = S.renderer(ts, "cuda")
    bidx, L = [1, 0], 6
    layers, cnt = lr.generate(bidx, scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, scd.faces_existence, L)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    g = np.random.RandomState(7)
    mat = dict(verts_color=g.uniform(0, 1, (P, 3)).astype(np.float32), faces_opacity=g.uniform(0.05, 0.95, F).astype(np.float32),
               faces_intense=g.uniform(0.5, 1.5, (2, F)).astype(np.float32), background=np.array([0.1, 0.3, 0.7], np.float32))
    dev = {k: torch.from_numpy(v).cuda() for k, v in mat.items()}
    color, depth, alpha = lr.render(bidx, layers, scd.verts, scd.faces, dev["verts_color"], dev["faces_opacity"], dev["faces_intense"],
                                    dev["background"], return_alpha=True)
    torch.cuda.synchronize()
    inp = G.inputs(lr, scd.verts, bidx)
    fwd = lref.forward32(layers.cpu(), ts.verts, ts.faces, mat["verts_color"], mat["faces_opacity"], mat["faces_intense"], inp["ndc"],
                         mat["background"], inp["ro"], inp["rd"])
    f32 = np.float32
    assert np.array_equal(color.cpu().numpy().view(np.uint32), fwd["color"].view(np.uint32))
    assert np.abs(depth.cpu().numpy() - (f32(1) - (fwd["depth_raw"] + f32(1)) / f32(2))).max() <= 1e-6
    assert np.abs(alpha.cpu().numpy() - (f32(1) - fwd["final_T"].reshape(alpha.shape))).max() <= 1e-6
    assert fwd["blend"].sum() > 1000 and (cnt > 0).float().mean() > 0.2


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def _args(W=20, H=12, B=2, dev="cuda"):
    ts, _ = S.case("holes", W, H)
    lr = S.renderer(ts)
    inp = G.inputs(lr, ts.verts, [0, 1][:B])
    t = lambda x: torch.from_numpy(x).to(dev)
    return [W, H, ts.verts.to(dev), ts.faces.to(dev), ts.tets.to(dev), ts.face_tets.to(dev), ts.tet_faces.to(dev),
            ts.faces_existence.to(dev), t(inp["ndc"]), t(inp["img"]), t(inp["ro"]), t(inp["rd"]), 3]


NAMES = ["width", "height", "verts", "faces", "tets", "face_tets", "tet_faces", "face_existence", "verts_ndc", "verts_image",
         "image_ray_o", "image_ray_d", "num_layers"]
SHAPE_MESSAGES = {"verts": r"verts must have dimensions \(P, 3\)", "faces": r"faces must have dimensions \(F, 3\)",
                  "tets": r"tets must have dimensions \(T, 4\)", "face_tets": r"face_tets must have dimensions \(F, 2\)",
                  "tet_faces": r"tet_faces must have dimensions \(T, 4\)", "face_existence": r"face_existence must have dimensions \(F,\)",
                  "verts_ndc": r"verts_ndc must have dimensions \(B, P, 3\)", "verts_image": r"verts_image must have dimensions \(B, P, 2\)",
                  "image_ray_o": r"image_ray_o must have dimensions \(B, H, W, 3\)",
                  "image_ray_d": r"image_ray_d must have dimensions \(B, H, W, 3\)"}


@pytest.mark.parametrize("which", list(SHAPE_MESSAGES))
def test_shape_messages(which):
    k = NAMES.index(which)
    for bad in ("rank", "last"):
        a = _args()
        a[k] = a[k][None] if bad == "rank" else torch.cat([a[k], a[k]], -1) if a[k].dim() > 1 else a[k][:-1]
        with pytest.raises(RuntimeError, match=SHAPE_MESSAGES[which]):
            _C.generate_render_layers_cuda(*a)


def test_cross_shape_messages():
    for k, rows, msg in ((5, -1, r"face_tets must have dimensions \(F, 2\)"), (6, -1, r"tet_faces must have dimensions \(T, 4\)"),
                         (9, None, "verts_ndc/verts_image shape mismatch"), (10, None, r"image_ray_o/image_ray_d must have dimensions")):
        a = _args()
        a[k] = a[k][:rows] if rows else a[k][:, :-1].contiguous()
        with pytest.raises(RuntimeError, match=msg):
            _C.generate_render_layers_cuda(*a)
    a = _args()
    a[12] = -1
    with pytest.raises(RuntimeError, match="num_layers must be non-negative"):
        _C.generate_render_layers_cuda(*a)
    a = _args()
    a[3] = a[3].to(torch.int64)
    with pytest.raises(RuntimeError, match="expected dtype"):
        _C.generate_render_layers_cuda(*a)


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.generate_render_layers_cuda(*_args(dev="cpu"))
    a = _args()
    a[7] = a[7].cpu()
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.generate_render_layers_cuda(*a)


def test_degenerate_sizes():
    """No pixels, no faces or no tets: the filled defaults (count 0, layers -1), and the library is not entered."""
    calls = []

    def spy(name):
        return lambda *a: calls.append(name) or 0

    with spy_library(dm2_layers_plan=spy("plan"), dm2_layers_run=spy("run")):
        for what in ("B", "W", "H", "F", "T"):
            a = _args()
            W, H, B, L = a[0], a[1], 2, a[12]
            if what == "B":
                for k in (8, 9, 10, 11):
                    a[k] = a[k][:0]
                B = 0
            elif what == "W":
                a[0] = W = 0
                a[10], a[11] = a[10][:, :, :0], a[11][:, :, :0]
            elif what == "H":
                a[1] = H = 0
                a[10], a[11] = a[10][:, :0], a[11][:, :0]
            elif what == "F":
                a[3], a[5], a[7] = a[3][:0], a[5][:0], a[7][:0]
            elif what == "T":
                a[4], a[6] = a[4][:0], a[6][:0]
            layers, cnt = _C.generate_render_layers_cuda(*a)
            assert tuple(layers.shape) == (B, H, W, L) and tuple(cnt.shape) == (B, H, W), what
            assert layers.dtype == torch.int32 and cnt.dtype == torch.int32
            assert (layers == -1).all() and (cnt == 0).all(), what
        assert not calls
