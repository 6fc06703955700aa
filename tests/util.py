"""Shared helpers for the tests (CPU side)."""
import contextlib
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dmesh2_renderer_amd as dm2  # noqa: E402
from dmesh2_renderer_amd import _C, scenes  # noqa: E402

ARG_NAMES = [
    "background", "patch_min", "patch_width", "patch_height", "verts", "faces", "verts_color",
    "faces_opacity", "verts_ndc", "verts_image", "faces_intense", "aa_temperature", "aa_face_verts",
    "aa_face_edges", "aa_face_edges_iszero", "aa_face_edges_recip", "aa_face_edges_normal",
    "aa_face_edges_normal_c", "len_oarea_buffer", "image_ray_o", "image_ray_d"]


def assert_own_exports(forward):
    """ABI v8: an op that travelled as a value code of another op's symbol has a forward and a backward export of its own,
    declared in the header, and the codes are gone from the header and from the shim."""
    hdr = open(os.path.join(ROOT, "include", "dm2_hip.h")).read()
    for name in (forward, forward + "_backward"):
        assert name in _C.EXPORTS and re.search(rf"^int {name}\(", hdr, flags=re.M), name
    for macro in ("DM2_TEX_VOLUME_", "DM2_TEX_HASH_GRID", "DM2_TEX_BOUNDARY_CUBE", "DM2_MIP_FILTER_CUBE_GGX"):
        assert macro not in hdr, macro
    for attr in ("TEX_HASH_GRID", "TEX_BOUNDARY_CUBE", "MIP_FILTER_CUBE_GGX", "hash_grid_code"):
        assert not hasattr(_C, attr), attr


@contextlib.contextmanager
def patched_C(**fns):
    """Temporarily replace functions of dmesh2_renderer_amd._C (capture / fake backends)."""
    old = {k: getattr(_C, k) for k in fns}
    try:
        for k, v in fns.items():
            setattr(_C, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(_C, k, v)


class _LibSpy:
    """The library with some entry points wrapped (render_forward_cuda looks it up once per call through load_library)."""

    def __init__(self, lib, **fns):
        self._lib = lib
        self.__dict__.update(fns)

    def __getattr__(self, name):
        return getattr(self._lib, name)


@contextlib.contextmanager
def spy_library(**fns):
    """``with spy_library(dm2_forward=f): ...`` -- the shim's calls of the named C entry points go to the given functions
    (which call the real ones of the yielded library as they see fit); every other entry point is the library's."""
    lib = _C.load_library()
    orig = _C.load_library
    _C.load_library = lambda: _LibSpy(lib, **fns)
    try:
        yield lib
    finally:
        _C.load_library = orig


def capture_forward_args(sc, batch_idx, patch_min, pw, ph, temp=1.0, K=20, device="cpu"):
    """Run the package's host prep (Renderer.forward) and return the 21 boundary args."""
    got = {}

    def fake(*args):
        got["args"] = args
        B = args[8].shape[0]
        z = torch.zeros
        return (0, z((B, ph, pw, 3), device=device), z((B, ph, pw), device=device), z(0), z(0), z(0), z(0), z(0), z(0), z(0))

    scd = sc.to(device)
    r = dm2.Renderer(scd.mv, scd.proj, sc.width, sc.height, device, aa_grad_buffer_size=K, tables_from_image=False)   # (the arguments are replayed as they are)
    with patched_C(render_forward_cuda=fake):
        r(batch_idx, torch.tensor(patch_min, dtype=torch.int64, device=device), pw, ph, scd.verts, scd.faces,
          scd.verts_color, scd.faces_opacity, scd.faces_intense[batch_idx], scd.background, aa_temperature=temp)
    return got["args"], r


def soup_args(W, H, F, seed, temp=1.0, K=20, cams=1, batch_idx=(0,), patch_min=None, pw=None, ph=None, shared=True,
              depth_complexity=4.0):
    sc = scenes.triangle_soup(W, H, F, seed, num_cams=cams, shared_verts=shared, depth_complexity=depth_complexity)
    batch_idx = list(batch_idx)
    if patch_min is None:
        patch_min = [[0, 0]] * len(batch_idx)
    return capture_forward_args(sc, batch_idx, patch_min, pw or W, ph or H, temp, K)[0], sc


def to_numpy_args(args):
    return [a.detach().cpu().numpy() if torch.is_tensor(a) else a for a in args]


def table_capacity():
    """LC_SLOTS of the layer kernels' per-block face table, read from dm2_face_table.h."""
    import re
    src = open(os.path.join(ROOT, "dmesh2_renderer_amd", "csrc", "dm2_face_table.h")).read()
    return int(re.search(r"constexpr int LC_SLOTS = (\d+);", src).group(1))


_REL_SEEN = []          # lists that collect every rel_linf computed while they are registered (watch_rel_linf)


def rel_linf(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    e = float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-12)) if a.size else 0.0
    for seen in _REL_SEEN:
        seen.append(e)
    return e


@contextlib.contextmanager
def watch_rel_linf():
    """``with watch_rel_linf() as seen:`` -- every value rel_linf returns inside the block, whoever calls it, is appended to
    ``seen`` (a test that runs another file's checks reports the worst of them)."""
    seen = []
    _REL_SEEN.append(seen)
    try:
        yield seen
    finally:
        _REL_SEEN.remove(seen)


def from_image_oracle_args(args):
    """The oracle's 21 arguments for a call whose AA tables are built from ``verts_image`` (DM2_FLAG_TABLES_FROM_IMAGE): args
    12-17 become the six tables the reference's ``Triangles`` builds from ``verts_image[:, faces]``, CCW reorder included
    (what the op's plan builds in registers).  Whatever ``args`` holds there, placeholders or tables, is ignored."""
    from oracle import cpu as orc
    na = to_numpy_args(args)
    vi, fc = na[9], na[5].astype(np.int64)
    Bv, Fv = vi.shape[0], fc.shape[0]
    t = orc.aa_tables(vi[:, fc.reshape(-1)].reshape(-1, 3, 2), np.float32, reorder=True)
    for k, name in zip(range(12, 17), ("verts", "edges", "iszero", "recip", "normal")):
        na[k] = t[name].reshape(Bv, Fv, 3, 2)
    na[17] = t["normal_c"].reshape(Bv, Fv, 3)
    return na


def scatter_aa_grad_to_verts(g_aa, aa_face_verts, verts_image, faces):
    """Per-corner gradient of the AA tables (B,F,3,2) -> per-vertex gradient of ``verts_image`` (B,P,2), summed in fp64.
    Corner 0 is always the face's vertex 0; corners 1 and 2 are its vertices 2 and 1 where the CCW reorder swapped them,
    which is where the table's corner 1 is not ``verts_image[faces[:, 1]]`` (the test the op's records make)."""
    g = np.asarray(g_aa, dtype=np.float64)
    av, vi, fc = np.asarray(aa_face_verts), np.asarray(verts_image), np.asarray(faces).astype(np.int64)
    B, F, P = g.shape[0], g.shape[1], vi.shape[1]
    v1 = vi[:, fc[:, 1]]                                                  # (B,F,2)
    swap = ~((av[:, :, 1, 0] == v1[..., 0]) & (av[:, :, 1, 1] == v1[..., 1]))
    idx = np.broadcast_to(fc, (B, F, 3)).copy()
    idx[..., 1] = np.where(swap, fc[:, 2], fc[:, 1])
    idx[..., 2] = np.where(swap, fc[:, 1], fc[:, 2])
    out = np.zeros((B, P, 2), dtype=np.float64)
    for b in range(B):
        np.add.at(out[b], idx[b].reshape(-1), g[b].reshape(-1, 2))
    return out


# ---- GPU side --------------------------------------------------------------------------------------------------------------
def pool_state(out):
    """What the forward ``out`` (its 10-tuple) left of its pair pool, read right after it (before any backward): dict(mode,
    claimed = pool slots its composite handed out (hit_valid[1]), bound = the plan's pair bound, cap = pool capacity of its
    binning buffer, hit_valid), or None when the forward kept no pool (mode != DM2_FWD_POOL)."""
    mode, bound = _C.last_forward_mode(), _C.last_pair_bound()
    R, bin_buf = out[0], out[8]
    if mode != _C.FWD_POOL or R <= 0:
        return None
    B, H, W = out[2].shape
    Tn = _C._tiles(B, W, H)
    lib = _C.load_library()
    cap = max(0, bin_buf.numel() - lib.dm2_scratch_bytes(_C.SCRATCH_BINNING, R, Tn)) // 4      # (as render_backward_cuda sizes it)
    hv = _C.debug_fetch(9, B * H * W, Tn, R, bin_buf, torch.int32, 4).cpu().numpy().view(np.uint32)
    return dict(mode=mode, claimed=int(hv[1]), bound=int(bound), cap=int(cap), hit_valid=hv.tolist())


def check_pool(state):
    """The pool invariant: the slots the composite claimed never exceed the plan's pair bound, nor the bound the pool."""
    if state is None:
        return
    assert state["hit_valid"][0] == 3, f"hit_valid {state['hit_valid']}: the forward reported DM2_FWD_POOL"
    assert state["claimed"] <= state["bound"] <= state["cap"], state


def run_from_image(args, dL_dcolor, dL_ddepth):
    """The op as bench.py runs its default path: placeholder AA tables (BandShardedOp(.., tables_from_image=True)), forward under
    ``tables_from_image`` + ``aa_grad_to_verts``.  Backward twice: the sixth gradient unrouted (B,F,3,2), then routed (B,P,2).
    ``args`` on the GPU.  -> (forward 10-tuple, six gradients (numpy), routed gradient (numpy), pool_state)."""
    from dmesh2_renderer_amd.sharding import BandShardedOp
    a = BandShardedOp(args, 1, 0, tables_from_image=True).args
    assert a[12].shape[1] == 0 and a[17].shape[1] == 0
    with _C.aa_grad_to_verts(True), _C.tables_from_image(True):
        out = _C.render_forward_cuda(*a)
    pool = pool_state(out)
    check_pool(pool)
    bw = (out[0], *a, dL_dcolor, dL_ddepth, out[7], out[8], out[9], out[3], out[4], out[5], out[6])
    with _C.tables_from_image(True):
        g = [x.cpu().numpy() for x in _C.render_backward_cuda(*bw)]
    with _C.aa_grad_to_verts(True), _C.tables_from_image(True):
        routed = _C.render_backward_cuda(*bw)[5].cpu().numpy()
    torch.cuda.synchronize()
    return out, g, routed, pool


GRAD_NAMES = ["verts", "verts_color", "faces_opacity", "verts_ndc", "faces_intense", "aa_face_verts"]
GRAD_TOL = 1e-5         # gradients: relative L-inf against the oracle (fp32 atomic summation order differs)


def to_dev(args, dev="cuda"):
    return [a.to(dev) if torch.is_tensor(a) else a for a in args]


def run_both(args, seed=0, backward=True, nthreads=1):
    """The HIP op and the oracle on the same 21 arguments (CPU tensors), forward and (with random output gradients drawn from
    ``seed``) backward.  -> dict(out, pool, ref[, grads, ref_grads])."""
    from oracle import cpu as orc
    dargs = to_dev(args)
    out = _C.render_forward_cuda(*dargs)
    res = dict(out=out, pool=pool_state(out))           # (read before any backward runs)
    ref = res["ref"] = orc.render_forward_cuda(*to_numpy_args(args), nthreads=nthreads)
    if backward:
        rng = np.random.RandomState(seed)
        gc = rng.randn(*ref.color.shape).astype(np.float32)
        gd = rng.randn(*ref.depth.shape).astype(np.float32)
        grads = _C.render_backward_cuda(out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(),
                                       out[7], out[8], out[9], out[3], out[4], out[5], out[6])
        res["grads"] = [g.cpu().numpy() for g in grads]
        res["ref_grads"] = orc.render_backward_cuda(ref, gc, gd, nthreads=nthreads)
    torch.cuda.synchronize()
    return res


def check_forward(res, args):
    """Forward bit-exact against the oracle: num_rendered, the pool invariant, ranges, face_list, final_T, final_prev_T,
    n_contrib, colour, depth, tri_cnt."""
    out, ref = res["out"], res["ref"]
    R, color, depth, oarea, tri_id, tri_cnt, doarea, face_buf, bin_buf, img_buf = out
    B, H, W = ref.depth.shape
    assert R == ref.num_rendered
    check_pool(res.get("pool"))                         # the pair pool held every pair the composite enumerated
    assert color.shape == (B, H, W, 3) and depth.shape == (B, H, W) and tri_cnt.shape == (B, H, W)
    assert oarea.dim() == 4 and tri_id.dim() == 4 and doarea.dim() == 6
    N, Tn = B * H * W, B * ((W + 15) // 16) * ((H + 15) // 16)
    if R > 0:
        ranges = _C.debug_fetch(0, N, Tn, R, img_buf, torch.int32, Tn * 2).cpu().numpy().view(np.uint32).reshape(Tn, 2)
        flist = _C.debug_fetch(1, N, Tn, R, bin_buf, torch.int32, R).cpu().numpy().view(np.uint32)
        assert np.array_equal(ranges, ref.binning.ranges)
        assert np.array_equal(flist, ref.binning.face_list)
        fT = _C.debug_fetch(2, N, Tn, R, img_buf, torch.float32, N).cpu().numpy()
        fpT = _C.debug_fetch(3, N, Tn, R, img_buf, torch.float32, N).cpu().numpy()
        nc = _C.debug_fetch(4, N, Tn, R, img_buf, torch.int32, N).cpu().numpy().view(np.uint32)
        flipped = int((nc != ref.n_contrib).sum())
        assert flipped == 0, f"{flipped} pixels with a different last contributor"
        assert np.array_equal(fT.view(np.uint32), ref.final_T.view(np.uint32))
        assert np.array_equal(fpT.view(np.uint32), ref.final_prev_T.view(np.uint32))
    c, d = color.cpu().numpy(), depth.cpu().numpy()
    assert np.array_equal(c.view(np.uint32), ref.color.view(np.uint32)), f"color max abs diff {np.abs(c - ref.color).max()}"
    assert np.array_equal(d.view(np.uint32), ref.depth.view(np.uint32)), f"depth max abs diff {np.abs(d - ref.depth).max()}"
    assert np.array_equal(tri_cnt.cpu().numpy(), ref.buf_tri_cnt)


def check_backward(res, tol=GRAD_TOL):
    """The six gradients within ``tol`` relative L-inf of the oracle's, the same non-finite pattern.  -> per-tensor worst."""
    worst = {}
    for name, g in zip(GRAD_NAMES, res["grads"]):
        r = res["ref_grads"][name]
        assert g.shape == r.shape, name
        assert np.isfinite(g).all() == np.isfinite(r).all(), name
        m = np.isfinite(r)
        worst[name] = rel_linf(g[m], r[m])
    assert all(v <= tol for v in worst.values()), worst
    ndc = res["grads"][3]
    assert not ndc[..., :2].any()                       # only the z channel receives gradient (backward.cu:516-518)
    return worst


def check_from_image(args, dL_dcolor, dL_ddepth, tol=1e-5, nthreads=1):
    """run_from_image against the oracle given the tables the reference builds from verts_image: num_rendered, colour, depth,
    tri_cnt, n_contrib bit-equal; the six gradients and the routed AA gradient (against the fp64 scatter of the oracle's) within
    ``tol`` relative L-inf.  -> per-tensor worst relative error."""
    from oracle import cpu as orc
    out, g, routed, _ = run_from_image(args, dL_dcolor, dL_ddepth)
    na = from_image_oracle_args(args)
    ref = orc.render_forward_cuda(*na, nthreads=nthreads)
    R = out[0]
    assert R == ref.num_rendered
    assert np.array_equal(out[1].cpu().numpy().view(np.uint32), ref.color.view(np.uint32))
    assert np.array_equal(out[2].cpu().numpy().view(np.uint32), ref.depth.view(np.uint32))
    assert np.array_equal(out[5].cpu().numpy(), ref.buf_tri_cnt)
    B, H, W = ref.depth.shape
    N, Tn = B * H * W, _C._tiles(B, W, H)
    if R > 0:
        nc = _C.debug_fetch(4, N, Tn, R, out[9], torch.int32, N).cpu().numpy().view(np.uint32)
        flipped = int((nc != ref.n_contrib.reshape(-1)).sum())
        assert flipped == 0, f"{flipped} pixels with a different last contributor"
    gref = orc.render_backward_cuda(ref, dL_dcolor.cpu().numpy(), dL_ddepth.cpu().numpy(), nthreads=nthreads)
    worst = {}
    for name, x in zip(GRAD_NAMES, g):
        assert x.shape == gref[name].shape, name
        worst[name] = rel_linf(x, gref[name])
    worst["aa_to_verts"] = rel_linf(routed, scatter_aa_grad_to_verts(gref["aa_face_verts"], na[12], na[9], na[5]))
    assert all(v <= tol for v in worst.values()), worst
    return worst


def per_pixel_terms_f64(args, gc, gd, pm, pw, ph):
    """Per gradient tensor: sum over the patch's pixels of |that pixel's contribution|, from the fp64 oracle run on
    1 x 1 patches -- the quantity an fp32 sum's rounding error scales with, whatever its order.
    (One view, the sum over the whole patch: what test_fuzz4_regression needs, kept as it was.  tests/upstream.py PixelTerms keeps
    the same terms per pixel and per output, sparse, so that many supports can be summed from one pass; it imports this module,
    so this function cannot be built on it.)"""
    from oracle import cpu as orc
    a = to_numpy_args(args)
    sabs = None
    for y in range(ph):
        for x in range(pw):
            b = list(a)
            b[1] = np.array([[pm[0][0] + x, pm[0][1] + y]], np.int32); b[2] = 1; b[3] = 1
            b[19] = np.ascontiguousarray(a[19][:, y:y + 1, x:x + 1]); b[20] = np.ascontiguousarray(a[20][:, y:y + 1, x:x + 1])
            r = orc.render_forward_cuda(*b, dtype=np.float64)
            gg = orc.render_backward_cuda(r, gc[:, y:y + 1, x:x + 1].astype(np.float64), gd[:, y:y + 1, x:x + 1].astype(np.float64))
            sabs = {n: np.abs(gg[n]) for n in GRAD_NAMES} if sabs is None else {n: sabs[n] + np.abs(gg[n]) for n in GRAD_NAMES}
    return sabs


EPS32 = 2.0 ** -24


def summation_bound(gmax, sabs):
    """The per-element acceptance test_gpu_coverage.py::test_fuzz4_regression derives: GRAD_TOL of the tensor's maximum plus
    8 eps32 times the sum of the absolute per-pixel terms (what any fp32 summation order is good to)."""
    return GRAD_TOL * gmax + 8.0 * EPS32 * sabs
