"""The oracle and the HIP kernels held to what the reference's own kernels compute.

oracle/build_ref.py compiles the reference project's kernels for gfx950 (tests/reference_lib.py loads them):
``strict`` without FMA contraction, as the oracle and the HIP kernels are built, and ``shipped`` with the compiler's default
contraction.  Neither is a CUDA build.  Here, on the very same argument tensors:

  forward   strict reference == oracle bit for bit: num_rendered, colour, depth, the four AA record tensors (whole tensors:
            both sides start from zeros), final_T, final_prev_T, n_contrib, tile ranges, face_list;
            HIP kernels (both work distributions) == strict reference bit for bit: num_rendered, colour, raw depth;
  backward  the strict reference's backward on its own forward's buffers against the oracle and against the HIP kernels in
            their default as-written dv mode: six gradients within 1e-5 relative L-inf of each tensor's maximum (the
            reference sums with float atomics in no fixed order, so bits are not available);
  layers    generate_render_layers_cuda: render_layers and render_layers_cnt exact, oracle and HIP kernels;
  shipped   how far contraction alone moves the reference (printed), and the HIP kernels against the shipped variant on the
            pixels where the two reference builds agree in their integer records.

Every test skips only where the reference modules were not built (reference_lib.load() is None).
"""
import functools

import numpy as np
import pytest
import torch

import far
import generate_ref as G
import reference_lib as RL
import structured
import tet_scenes as S
from util import GRAD_NAMES, _C, capture_forward_args, rel_linf, scenes, soup_args, to_numpy_args

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # gradients: relative L-inf of each tensor's maximum (the project's figure)
DEV = "cuda:0"


def _ref(variant="strict"):
    mod = RL.load(variant)
    if mod is None:
        pytest.skip("oracle/_ref/ holds no reference build")
    return mod


# ---- scenes: name -> the 21 boundary arguments (CPU tensors) ---------------------------------------------------------------
def _soup(temp, K):
    return soup_args(96, 64, 400, scenes.SEED_BASE + 42, temp=temp, K=K)[0]          # (smoke()'s scene)


def _two_views():
    """A 40 x 24 patch (no multiple of 16 either way) of a 96 x 64 frame, two cameras, each with its own patch_min."""
    return soup_args(96, 64, 400, scenes.SEED_BASE + 43, temp=1.0, K=20, cams=2, batch_idx=(0, 1),
                     patch_min=[[8, 5], [37, 23]], pw=40, ph=24)[0]


def _ties():
    """tests/test_gpu_binning.py's tie scene: every face four times, so equal depth keys whose order is the face id."""
    sc = scenes.triangle_soup(64, 64, 700, scenes.SEED_BASE + 700 + len("ties"), num_cams=1, shared_verts=False, depth_complexity=8.0)
    sc.faces = sc.faces.repeat(4, 1)
    sc.faces_opacity = sc.faces_opacity.repeat(4)
    sc.faces_intense = sc.faces_intense.repeat(1, 4)
    return capture_forward_args(sc, [0], [[0, 0]], 64, 64, 1.0, 20)[0]


def _far():
    """tests/far.py's scene with the camera inside the lattice (vertices 1e5 .. 1e6 px out, clamped w, faces through the
    frustum's side) -- without the 37 faces over which the reference's binning races (reference_lib.races_in_binning: dropped
    by the z test, yet with a tile rectangle; the oracle and the op drop them in both kernels, so they contribute nothing
    there, while the reference's lists depend on thread order).  Every other face stays."""
    sc = far.inside_scene(64, 48, 5, n=3)
    a = list(capture_forward_args(sc, [0], [[0, 0]], 64, 48, 1.0, 20)[0])
    n = to_numpy_args(a)
    keep = torch.from_numpy(~RL.races_in_binning(n[5], n[8], n[9], n[1], 64, 48)[0])
    assert 0 < int((~keep).sum()) < 100
    a[5], a[7], a[10] = a[5][keep].contiguous(), a[7][keep].contiguous(), a[10][:, keep].contiguous()
    for k in range(12, 18):
        a[k] = a[k][:, keep].contiguous()
    return a


def _empty():
    """No face reaches the frame, num_rendered 0: every vertex 1e4 px to the right of it (not behind the far plane: faces the
    z test drops while their rectangle is not empty are where the reference's binning races, see _far)."""
    a = list(_soup(1.0, 20))
    a[9] = a[9] + torch.tensor([1.0e4, 0.0])
    return a


SCENES = {
    "soup_t1": lambda: _soup(1.0, 20),
    "soup_t05": lambda: _soup(0.5, 20),
    "soup_t0": lambda: _soup(0.0, 20),
    "soup_k2": lambda: _soup(1.0, 2),                 # the record stack overflows: its pop rule runs
    "two_views": _two_views,
    "ties": _ties,
    "aligned": lambda: structured.make_args("grid"),
    "degenerate": lambda: structured.make_args("degenerate"),
    "far": _far,
    "empty": _empty,
}
BACKWARD_SCENES = ("soup_t0", "soup_t05", "soup_t1", "soup_k2", "ties", "two_views")


@functools.lru_cache(maxsize=None)
def _args(name):
    return tuple(SCENES[name]())


@functools.lru_cache(maxsize=None)
def _oracle_forward(name):
    """The oracle's forward of scene ``name``: computed once, read-only."""
    from oracle import cpu as orc
    with np.errstate(all="ignore"):
        return orc.render_forward_cuda(*to_numpy_args(_args(name)), nthreads=min(orc.max_threads(), 16))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    n = int((_bits(a) != _bits(b)).sum())
    assert n == 0, f"{what}: {n} of {a.size} entries differ"


class _flags:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.old = _C.set_flags(self.flags)

    def __exit__(self, *exc):
        _C.set_flags(self.old)


def _seeded_grads(shape_c, shape_d, seed=0):
    rng = np.random.RandomState(seed)
    return rng.randn(*shape_c).astype(np.float32), rng.randn(*shape_d).astype(np.float32)


# ---- 4a: forward, strict reference against the oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_reference_equals_oracle(name):
    mod = _ref()
    dargs = RL.to_device(_args(name), DEV)
    ref = RL.Forward(mod, dargs)
    orc = _oracle_forward(name)
    if name == "empty":
        assert orc.num_rendered == 0
    elif name == "soup_k2":
        assert _oracle_forward("soup_t1").buf_tri_cnt.max() > 2 == orc.buf_tri_cnt.max(), "the scene must overflow a 2-slot record stack"
    assert ref.num_rendered == orc.num_rendered
    _same(ref.color, orc.color, "colour")
    _same(ref.depth, orc.depth, "depth")
    _same(ref.tri_cnt, orc.buf_tri_cnt, "tri_cnt")
    _same(ref.tri_id, orc.buf_tri_id, "tri_id")
    _same(ref.oarea, orc.buf_oarea, "oarea")
    _same(ref.doarea, orc.buf_doarea, "doarea")
    _same(ref.image["final_T"], orc.final_T, "final_T")
    _same(ref.image["final_prev_T"], orc.final_prev_T, "final_prev_T")
    _same(ref.image["n_contrib"], orc.n_contrib, "n_contrib")
    _same(ref.image["ranges"], orc.binning.ranges, "ranges")
    _same(ref.face_list, orc.binning.face_list, "face_list")


# ---- 4b: HIP kernels against the strict reference --------------------------------------------------------------------------
@pytest.mark.parametrize("legacy", [False, True], ids=["default", "legacy"])
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_kernels_equal_reference(name, legacy):
    mod = _ref()
    dargs = RL.to_device(_args(name), DEV)
    ref = RL.Forward(mod, dargs)
    with _flags(_C.DM2_FLAG_LEGACY_KERNELS if legacy else 0):
        out = _C.render_forward_cuda(*dargs)
        torch.cuda.synchronize()
    assert out[0] == ref.num_rendered
    _same(out[1].cpu().numpy(), ref.color, "colour")
    _same(out[2].cpu().numpy(), ref.depth, "raw depth")


# ---- 4c: backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKWARD_SCENES)
def test_backward_reference_defines_gradients(name):
    from oracle import cpu as orc_mod
    mod = _ref()
    dargs = RL.to_device(_args(name), DEV)
    ref = RL.Forward(mod, dargs)
    gc, gd = _seeded_grads(ref.color.shape, ref.depth.shape, seed=len(name))
    dgc, dgd = torch.from_numpy(gc).to(DEV), torch.from_numpy(gd).to(DEV)
    g_ref = RL.backward(mod, ref, dgc, dgd)
    with np.errstate(all="ignore"):
        g_orc = orc_mod.render_backward_cuda(_oracle_forward(name), gc, gd, nthreads=min(orc_mod.max_threads(), 16))
    with _flags(0):                                           # as-written dv: DM2_FLAG_CORRECTED_DV off
        out = _C.render_forward_cuda(*dargs)
        g_hip = [g.cpu().numpy() for g in _C.render_backward_cuda(out[0], *dargs, dgc, dgd, out[7], out[8], out[9], out[3],
                                                                  out[4], out[5], out[6])]
        torch.cuda.synchronize()
    worst = {}
    for k, nm in enumerate(GRAD_NAMES):
        r = g_ref[k]
        assert np.isfinite(r).all(), nm
        assert g_orc[nm].shape == r.shape == g_hip[k].shape, nm
        worst[nm] = (rel_linf(g_orc[nm], r), rel_linf(g_hip[k], r))
    print(f"\n[reference backward] {name}: rel L-inf (oracle, kernels) " + ", ".join(f"{k} {a:.2e}/{b:.2e}" for k, (a, b) in worst.items()))
    assert any(np.abs(g).max() > 0 for g in g_ref)
    assert all(a <= TOL and b <= TOL for a, b in worst.values()), worst


# ---- 4d: layers ------------------------------------------------------------------------------------------------------------
# The image is padded to multiples of the 16 x 16 tile on purpose.  The reference's first-intersection kernel initialises
# first_face / first_tet from EVERY thread of a tile, also from those beyond the image's right and bottom edge: their index
# W * y + x names another pixel (a race with that pixel's own result) or lies past the end of the buffer (an out-of-bounds
# store).  At other sizes the reference's layers are therefore not defined, and reference_lib refuses to run them.  The
# scenes of tests/tet_scenes.py need their odd sizes (aligned: the central ray in a lattice plane), so they keep them and the
# ray tensors grow to the next multiple of 16 by repeating the last column and row: the tile grid, the tile lists and every
# original pixel's ray are unchanged, the added pixels are ordinary pixels, and all three implementations get the same
# padded arguments.  What the op does at odd sizes stays with tests/test_gpu_generate.py and the oracle.
LAYER_SCENES = ("lattice", "holes", "duplicates", "aligned", "inside")
LAYER_LS = (1, 4, 8)


@functools.lru_cache(maxsize=None)
def _tet_scene(name):
    if name == "lattice":
        return scenes.tet_lattice(64, 48, 3, seed=scenes.SEED_BASE + 3, num_cams=2)
    return S.case(name)[0]


def _bidx(ts, B):
    last = ts.mv.shape[0] - 1
    return [0] if B == 1 else [last, 0, last]


def _layer_args(ts, bidx, existence, L):
    """The 13 arguments of generate_render_layers_cuda as LayeredRenderer.generate hands them over (CPU tensors), the ray
    tensors and the image size padded to multiples of 16 (see above)."""
    lr = S.renderer(ts, "cpu")
    inp = G.inputs(lr, ts.verts, bidx)
    t = torch.from_numpy
    W16, H16 = -(-ts.width // 16) * 16, -(-ts.height // 16) * 16
    pad = ((0, 0), (0, H16 - ts.height), (0, W16 - ts.width), (0, 0))
    fc = ts.faces.numpy()
    if RL.races_in_binning(fc, inp["ndc"], inp["img"], np.zeros((len(bidx), 2), np.float32), W16, H16).any():
        # holes' second camera and both cameras of inside (the camera is in the mesh) have faces that the z test drops although
        # their tile rectangle is not empty: the reference's binning races over them (reference_lib.races_in_binning).  With ndc z
        # clamped to [-1, 1] the z test drops nothing; the rays, the geometry and so the walks are the scene's, the clamp is
        # monotone in depth, and all three implementations get the same clamped argument.
        inp = dict(inp, ndc=np.concatenate([inp["ndc"][..., :2], np.clip(inp["ndc"][..., 2:], -1.0, 1.0)], -1))
        assert not RL.races_in_binning(fc, inp["ndc"], inp["img"], np.zeros((len(bidx), 2), np.float32), W16, H16).any()
    inp = dict(inp, ro=np.ascontiguousarray(np.pad(inp["ro"], pad, mode="edge")), rd=np.ascontiguousarray(np.pad(inp["rd"], pad, mode="edge")))
    return [W16, H16, ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, t(np.asarray(existence, np.int32)),
            t(inp["ndc"]), t(inp["img"]), t(inp["ro"]), t(inp["rd"]), L]


def _existence(ts, which):
    F = ts.faces.shape[0]
    return S.existence_tables(F, 11)[which]


@pytest.mark.parametrize("table", ["ones", "odd"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", LAYER_SCENES)
def test_layers_reference_equals_oracle_and_kernels(name, B, table):
    from oracle import cpu as orc_mod
    mod = _ref()
    ts = _tet_scene(name)
    ex = _existence(ts, table)
    for L in LAYER_LS:
        a = _layer_args(ts, _bidx(ts, B), ex, L)
        da = RL.to_device(a, DEV)
        rl, rc = RL.generate_layers(mod, da)
        ol, oc = orc_mod.generate_render_layers_cuda(*to_numpy_args(a), nthreads=min(orc_mod.max_threads(), 16))
        with _flags(0):
            hl, hc = (x.cpu().numpy() for x in _C.generate_render_layers_cuda(*da))
        assert rc.max() >= 1, "the scene must produce layers"
        _same(oc, rc, f"L={L} oracle render_layers_cnt")
        _same(ol, rl, f"L={L} oracle render_layers")
        _same(hc, rc, f"L={L} kernels render_layers_cnt")
        _same(hl, rl, f"L={L} kernels render_layers")


# ---- 4e: the shipped variant -----------------------------------------------------------------------------------------------
MAX_EXCLUDED = 0.01            # share of pixels per scene whose integer records differ between the two reference builds


def test_shipped_variant_soup():
    """The soup at temperature 1 under both reference builds: what contraction alone moves (printed; DESIGN.md §2 holds the
    figures), then the HIP kernels against the shipped build on the pixels whose integer records (tri_cnt, tri_id, n_contrib)
    agree between the two builds -- within 1e-5 of each tensor's maximum, or twice the strict-against-shipped deviation where
    that alone exceeds 1e-5 (a reference-against-reference figure).  The output gradients are zero on the excluded pixels for
    every backward, so that the gradients compare on the same pixels."""
    strict, shipped = _ref("strict"), _ref("shipped")
    dargs = RL.to_device(_args("soup_t1"), DEV)
    fs, fh = RL.Forward(strict, dargs), RL.Forward(shipped, dargs)
    B, H, W = fs.depth.shape
    assert fs.num_rendered == fh.num_rendered
    differ = (fs.tri_cnt != fh.tri_cnt) | (fs.tri_id != fh.tri_id).any(-1) \
        | (fs.image["n_contrib"] != fh.image["n_contrib"]).reshape(B, H, W)
    share = float(differ.mean())
    keep = ~differ
    dev = {"color": rel_linf(fh.color[keep], fs.color[keep]), "depth": rel_linf(fh.depth[keep], fs.depth[keep])}
    dev_all = {"color": rel_linf(fh.color, fs.color), "depth": rel_linf(fh.depth, fs.depth)}

    gc, gd = _seeded_grads(fs.color.shape, fs.depth.shape, seed=5)
    gc[differ] = 0.0
    gd[differ] = 0.0
    dgc, dgd = torch.from_numpy(gc).to(DEV), torch.from_numpy(gd).to(DEV)
    gs, gh = RL.backward(strict, fs, dgc, dgd), RL.backward(shipped, fh, dgc, dgd)
    for k, nm in enumerate(GRAD_NAMES):
        dev["grad " + nm] = rel_linf(gh[k], gs[k])
    print(f"\n[shipped vs strict] soup 96x64 temperature 1: excluded pixels {int(differ.sum())} of {differ.size} ({share:.4%}); "
          + "rel L-inf on the kept pixels: " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items())
          + f"; on all pixels: colour {dev_all['color']:.3e}, depth {dev_all['depth']:.3e}")
    assert share <= MAX_EXCLUDED, f"{share:.4%} of the pixels differ in their integer records between the two reference builds"

    with _flags(0):
        out = _C.render_forward_cuda(*dargs)
        g = [x.cpu().numpy() for x in _C.render_backward_cuda(out[0], *dargs, dgc, dgd, out[7], out[8], out[9], out[3], out[4],
                                                              out[5], out[6])]
        torch.cuda.synchronize()
    got = {"color": rel_linf(out[1].cpu().numpy()[keep], fh.color[keep]), "depth": rel_linf(out[2].cpu().numpy()[keep], fh.depth[keep])}
    for k, nm in enumerate(GRAD_NAMES):
        got["grad " + nm] = rel_linf(g[k], gh[k])
    tol = {k: (TOL if dev[k] <= TOL else 2.0 * dev[k]) for k in dev}
    print("[kernels vs shipped] " + ", ".join(f"{k} {v:.3e} (tol {tol[k]:.1e})" for k, v in got.items()))
    assert out[0] == fh.num_rendered
    assert all(got[k] <= tol[k] for k in got), {k: (got[k], tol[k]) for k in got if got[k] > tol[k]}


def test_shipped_variant_lattice():
    """The lattice under both reference builds: the number of layer entries contraction alone changes (printed), at most 1 %
    of the pixels; on the others the HIP kernels' layers equal the shipped build's."""
    strict, shipped = _ref("strict"), _ref("shipped")
    ts = _tet_scene("lattice")
    da = RL.to_device(_layer_args(ts, [0], _existence(ts, "ones"), 8), DEV)
    sl, sc_ = RL.generate_layers(strict, da)
    hl, hc = RL.generate_layers(shipped, da)
    differ = (sl != hl).any(-1) | (sc_ != hc)
    print(f"\n[shipped vs strict] lattice 64x48 L=8: {int((sl != hl).sum())} of {sl.size} layer entries and "
          f"{int((sc_ != hc).sum())} of {sc_.size} counts differ; pixels {int(differ.sum())} ({float(differ.mean()):.4%})")
    assert float(differ.mean()) <= MAX_EXCLUDED
    with _flags(0):
        kl, kc = (x.cpu().numpy() for x in _C.generate_render_layers_cuda(*da))
    keep = ~differ
    _same(kc[keep], hc[keep], "kernels render_layers_cnt against the shipped build")
    _same(kl[keep], hl[keep], "kernels render_layers against the shipped build")
