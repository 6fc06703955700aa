"""The composite kernels' per-pair phases as straight-line code (dm2_clip_area.h, clamp_bary_uv, phase B2 of
dm2_forward_queue.hip): every predicate site and select of the rewrite, reached by scenes built here and held to the oracle.

1. Hand-built scenes on a 16 x 16 frame (one tile) and a 40 x 24 frame (partial tiles on both axes), <= 64 faces.  Image space
   and world space coincide (world vertex = (x_img, y_img, z), the ray of pixel (x, y) starts at (x + 0.5, y + 0.5, 0) and
   runs along +z), so a pair's (u, v) are the barycentrics of the pixel centre.  ``present`` asserts from that geometry alone,
   in float64 numpy, that every case is there before anything is compared.
2. clamp_bary_uv on its region boundaries: one large face, caller-supplied rays that put (u, v) exactly on u = 0, v = 0,
   u = 1, v = 1, u + v = 1, v = u - 1 and v = u + 1; a second face with a NaN image vertex.
3. Nothing moved: the forward's five outputs against arrays written once by the library of the commit named in the file
   (tests/golden/straightline_*.npz), bit for bit."""
import contextlib
import os

import numpy as np
import pytest
import torch

from util import GRAD_NAMES, GRAD_TOL, ROOT, check_backward, check_forward, check_from_image, rel_linf, run_both, to_dev, \
    to_numpy_args

from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FRAMES = {"16x16": (16, 16), "40x24": (40, 24)}


def _orc():
    from oracle import cpu as orc
    return orc


@contextlib.contextmanager
def _flags(f):
    old = _C.set_flags(f)
    try:
        yield
    finally:
        _C.set_flags(old)


# ---- geometry, float64, no library involved ---------------------------------------------------------------------------------
CORNERS = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])        # aa.h:103-149: (min,min) (max,min) (max,max) (min,max)


def _edge_side(tri, p):
    """(3,) signed cross products of the triangle's edges i -> i+1 with p - v_i (same sign everywhere: p inside)."""
    a, b = tri, np.roll(tri, -1, axis=0)
    return (b[:, 0] - a[:, 0]) * (p[1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (p[0] - a[:, 0])


def _inside(tri, p, orient):
    return bool((_edge_side(tri, p) * orient > 0).all())


def _bary_uv(tri, p):
    """Moeller-Trumbore (auxiliary.h:212-243) for the ray (p, 0) + t (0, 0, 1) and the world triangle (tri, z): u, v."""
    p0, p1, p2 = [np.array([tri[i, 0], tri[i, 1], 1.0]) for i in range(3)]
    ro, rd = np.array([p[0], p[1], 0.0]), np.array([0.0, 0.0, 1.0])
    T, E1, E2 = ro - p0, p1 - p0, p2 - p0
    P, Q = np.cross(rd, E2), np.cross(T, E1)
    den = P @ E1
    return (P @ T) / den, (Q @ rd) / den


def _region(u, v, margin=1e-4):
    """clamp_bary_uv's region (auxiliary.h:292-329) of (u, v), or -1 within ``margin`` of a boundary between regions."""
    lines = (u, v, u - 1.0, v - 1.0, u + v - 1.0, v - (u - 1.0), v - (u + 1.0))
    if min(abs(x) for x in lines) < margin:
        return -1
    if u >= 0 and v >= 0 and u + v <= 1: return 0
    if u <= 0 and v <= 0: return 1
    if (u >= 1 and v <= 0) or (v >= 0 and v <= u - 1): return 2
    if (u <= 0 and v >= 1) or (u >= 0 and v >= u + 1): return 3
    if u <= 0 and 0 <= v <= 1: return 4
    if 0 <= u <= 1 and v <= 0: return 5
    return 6


def _pair_cases(tri, W, H):
    """Per pixel of the frame the triangle's bbox touches: (x, y, corners inside, exit edge or -1, region or -1, area > 0).
    Exit edge: the inside corners of a partly covered pixel form one counter-clockwise run; the reference's corner walk
    (aa.h:359-379) enters it behind the crossing of the pixel edge from the corner before the run to its first corner, and the
    triangle edge that crosses there last is the one whose polygon corners come right before the walk."""
    orient = np.sign(_edge_side(tri, tri.mean(axis=0))[0])
    x0, x1 = int(np.floor(tri[:, 0].min())), int(np.ceil(tri[:, 0].max()))
    y0, y1 = int(np.floor(tri[:, 1].min())), int(np.ceil(tri[:, 1].max()))
    out = []
    for y in range(max(0, y0), min(H, y1)):
        for x in range(max(0, x0), min(W, x1)):
            org = np.array([x, y], dtype=np.float64)
            ins = [_inside(tri, org + c, orient) for c in CORNERS]
            n = sum(ins)
            vert_in = any(x < vx < x + 1 and y < vy < y + 1 for vx, vy in tri)
            exit_edge = -1
            starts = [c for c in range(4) if ins[c] and not ins[(c - 1) & 3]]
            if 1 <= n <= 3 and len(starts) == 1:
                c0 = starts[0]
                a, b = org + CORNERS[(c0 - 1) & 3], org + CORNERS[c0]            # outside -> inside along one pixel edge
                best = None
                for i in range(3):
                    sa, sb = _edge_side(tri, a)[i] * orient, _edge_side(tri, b)[i] * orient
                    if sa < 0 < sb:
                        t = sa / (sa - sb)                                       # where edge i's line crosses a -> b
                        if best is None or t > best[0]:
                            best = (t, i)
                exit_edge = best[1] if best else -1
            u, v = _bary_uv(tri, org + 0.5)
            out.append((x, y, n, exit_edge, _region(u, v), n > 0 or vert_in))
    return out


# ---- the scenes -------------------------------------------------------------------------------------------------------------
def _special_faces(ox, oy):
    """Hand-placed faces (shifted by whole pixels, which keeps the exact ones exact)."""
    s = [
        [(2.2, 2.3), (2.7, 2.4), (2.4, 2.8)],                    # inside one pixel
        [(0.5, 8.5), (7.5, 8.7), (1.0, 15.5)],                   # covers several pixels fully
        [(9.25, 1.25), (12.75, 1.25), (9.25, 4.75)],             # one horizontal and one vertical edge (e = 0 exactly)
        [(9.3, 6.2), (12.6, 6.2005), (10.1, 8.9)],               # an "iszero" edge: |e.y| = 5e-4 < 1e-3
        [(5.0, 3.3), (7.4, 4.1), (5.6, 5.7)],                    # a vertex on a pixel line
        [(12.0, 10.0), (14.5, 10.75), (12.5, 13.25)],            # a vertex on a pixel corner
        [(2.5, 4.5), (4.5, 6.5), (2.25, 6.5)],                   # an edge through the pixel corners (3, 5) and (4, 6)
        [(8.5, 12.0), (11.5, 12.0), (10.0, 14.5)],               # an edge along a pixel line
    ]
    return [np.array(t, dtype=np.float64) + np.array([ox, oy], dtype=np.float64) for t in s]


def _choose_faces(W, H, seed):
    """Random small triangles (0.3 .. 3.5 px), greedily kept while they add a (corners inside, exit edge) combination or a
    clamp region not yet seen, then any up to 36; then the hand-placed ones."""
    rng = np.random.default_rng(seed)
    want = {("walk", n, e) for n in (1, 2, 3) for e in range(3)} | {("region", r) for r in range(7)}
    faces = []
    for _ in range(4000):
        if not want and len(faces) >= 36:
            break
        c = rng.uniform([1.0, 1.0], [W - 1.0, H - 1.0])
        size = rng.choice([0.3, 0.8, 1.5, 2.5, 3.5])
        tri = c + rng.uniform(-size, size, (3, 2))
        tri = np.round(tri * 64.0) / 64.0 + 1.0 / 256.0             # (exact in float32, never on a pixel line)
        if abs(_edge_side(tri, tri[2])[0]) < 0.05:                 # (a sliver)
            continue
        if _edge_side(tri, tri[2])[0] < 0:
            tri = tri[[0, 2, 1]]
        got = set()
        for x, y, n, e, r, pos in _pair_cases(tri, W, H):
            if e >= 0: got.add(("walk", n, e))
            if r >= 0 and pos: got.add(("region", r))
        if got & want or not want:
            want -= got
            faces.append(tri)
    assert not want, want
    return faces + _special_faces(W - 16, H - 16)


def build_scene(frame, classes=False, temp=1.0, nan_face=False):
    """The 21 boundary arguments (CPU tensors) of the frame's scene, and its image-space triangles in table order."""
    orc = _orc()
    W, H = FRAMES[frame]
    tris = _choose_faces(W, H, 7 if frame == "16x16" else 8)
    if classes:                                                     # ten faces over the whole frame: >= 32 candidate pairs per entry
        for k in range(10):
            tris.append(np.array([(-3.5 - k, -2.25), (2.0 * W + 4.5 + k, -1.5 - k), (-2.5, 2.0 * H + 3.25 + k)]))
    tri = np.stack(tris).astype(np.float32)
    t = orc.aa_tables(tri.copy(), np.float32, reorder=True)
    tri = np.asarray(t["verts"], dtype=np.float32).reshape(-1, 3, 2)   # table order = vertex order: the world faces never swap
    F = tri.shape[0]
    assert F <= 64
    rng = np.random.default_rng(99)
    z = 1.0 + 0.01 * np.arange(F, dtype=np.float32)
    verts = np.concatenate([tri.reshape(-1, 2), np.repeat(z, 3)[:, None]], axis=1).astype(np.float32)
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    vimg = tri.reshape(1, -1, 2).copy()
    ndc = np.stack([vimg[0, :, 0] * 2 / W - 1, vimg[0, :, 1] * 2 / H - 1, np.repeat(-0.5 + 0.01 * np.arange(F), 3)], axis=1)
    opac = rng.uniform(0.2, 0.6, F).astype(np.float32)
    if classes:
        opac[-10:] = 0.05
    if nan_face:
        vimg[0, 3 * (F - 1) + 1, 0] = np.nan
    t = orc.aa_tables(vimg[0].reshape(F, 3, 2).copy(), np.float32, reorder=not nan_face)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ray_o = np.stack([xs + 0.5, ys + 0.5, np.zeros_like(xs)], axis=-1)[None]
    ray_d = np.broadcast_to(np.array([0, 0, 1], np.float32), ray_o.shape).copy()
    T = torch.from_numpy
    args = [T(rng.uniform(0, 1, 3).astype(np.float32)), torch.zeros((1, 2), dtype=torch.int32), W, H, T(verts), T(faces),
            T(rng.uniform(0, 1, (3 * F, 3)).astype(np.float32)), T(opac), T(ndc[None].astype(np.float32)), T(vimg),
            T(rng.uniform(0.5, 1.0, (1, F)).astype(np.float32)), float(temp)]
    for name in ("verts", "edges", "iszero", "recip", "normal"):
        args.append(T(np.ascontiguousarray(t[name]).reshape(1, F, 3, 2)))
    args += [T(np.ascontiguousarray(t["normal_c"]).reshape(1, F, 3)), 20, T(ray_o), T(ray_d)]
    return args, tri.astype(np.float64)


def present(tri, W, H):
    """Every case the rewrite touches is in the scene: asserted from the geometry (float64), nothing else."""
    walks, regions, full, sub = set(), set(), 0, False
    for f in tri:
        cases = _pair_cases(f, W, H)
        for x, y, n, e, r, pos in cases:
            if e >= 0: walks.add((n, e))
            if r >= 0 and pos: regions.add(r)
            full += n == 4
        sub |= np.ptp(f[:, 0]) < 1 and np.ptp(f[:, 1]) < 1 and np.floor(f[:, 0].min()) == np.floor(f[:, 0].max())
    assert walks == {(n, e) for n in (1, 2, 3) for e in range(3)}, walks
    assert regions == set(range(7)), regions
    assert full >= 3 and sub
    size = np.maximum(np.ptp(tri[:, :, 0], axis=1), np.ptp(tri[:, :, 1], axis=1))
    assert ((size > 2) & (size < 3.5)).any()                                              # 2-3 px faces
    e = np.roll(tri, -1, axis=1) - tri
    assert (e == 0).any() and ((np.abs(e) < 1e-3) & (e != 0)).any()                       # axis-parallel and "iszero" edges
    on_line = (tri == np.round(tri)) & (tri > 0) & (tri < np.array([W, H]))
    assert on_line.any() and on_line.all(axis=2).any()                                    # a vertex on a pixel line / corner
    through = False                                                                       # an edge through a pixel corner
    for f in tri:
        for i in range(3):
            a, b = f[i], f[(i + 1) % 3]
            for cx in range(int(np.ceil(min(a[0], b[0]))), int(np.floor(max(a[0], b[0]))) + 1):
                for cy in range(int(np.ceil(min(a[1], b[1]))), int(np.floor(max(a[1], b[1]))) + 1):
                    strictly = 0 < cx < W and 0 < cy < H and (cx, cy) != tuple(a) and (cx, cy) != tuple(b)
                    through |= strictly and (b[0] - a[0]) * (cy - a[1]) - (b[1] - a[1]) * (cx - a[0]) == 0
    assert through


_SCENES = {}


def _scene(frame, classes=False, temp=1.0):
    key = (frame, classes, temp)
    if key not in _SCENES:
        args, tri = build_scene(frame, classes, temp)
        W, H = FRAMES[frame]
        present(tri[:len(tri) - (10 if classes else 0)], W, H)
        _SCENES[key] = args
    return _SCENES[key]


def _check_classes(out, classes):
    assert (_C.last_pair_bound() >= 32 * out[0]) == classes, (_C.last_pair_bound(), out[0])


# ---- 1. the scenes through every route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [False, True], ids=["single", "classes"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_scene_default_route(frame, classes):
    args = _scene(frame, classes)
    res = run_both(args, seed=3)
    assert _C.last_forward_mode() == _C.FWD_POOL
    _check_classes(res["out"], classes)
    check_forward(res, args)
    check_backward(res)
    assert np.abs(res["grads"][5]).max() > 0


@pytest.mark.parametrize("classes", [False, True], ids=["single", "classes"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_scene_without_pair_pool(frame, classes):
    """DM2_FLAG_NO_PAIR_POOL: masks only, the CLIP instantiation of the backward."""
    args = _scene(frame, classes)
    with _flags(_C.DM2_FLAG_NO_PAIR_POOL):
        res = run_both(args, seed=4)
        assert _C.last_forward_mode() == _C.FWD_MASKS
    check_forward(res, args)
    check_backward(res)


@pytest.mark.parametrize("frame", list(FRAMES))
def test_scene_temperature_zero(frame):
    args = _scene(frame, False, 0.0)
    res = run_both(args, seed=5)
    assert _C.last_forward_mode() == _C.FWD_POINT
    check_forward(res, args)
    check_backward(res)


@pytest.mark.parametrize("classes", [False, True], ids=["single", "classes"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_scene_tables_from_image(frame, classes):
    """Placeholder AA tables, built by the plan from verts_image (the benchmarked route)."""
    args = _scene(frame, classes)
    W, H = FRAMES[frame]
    rng = np.random.default_rng(6)
    gc = torch.from_numpy(rng.standard_normal((1, H, W, 3)).astype(np.float32)).cuda()
    gd = torch.from_numpy(rng.standard_normal((1, H, W)).astype(np.float32)).cuda()
    check_from_image(to_dev(args), gc, gd)


@pytest.mark.parametrize("classes", [False, True], ids=["single", "classes"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_scene_face_weights(frame, classes):
    """The WEIGHTS instantiations of the forward: the ten outputs as without the weights, the weights as the oracle's."""
    from test_gpu_face_weights import check_weights, oracle_weights
    orc = _orc()
    args = _scene(frame, classes)
    want, _ = oracle_weights(to_numpy_args(args))
    with _C.face_weights_output(True):
        out = _C.render_forward_cuda(*to_dev(args))
    _check_classes(out, classes)
    check_forward(dict(out=out[:10], ref=orc.render_forward_cuda(*to_numpy_args(args))), args)
    check_weights(out[10], want)


@pytest.mark.parametrize("pool", [True, False], ids=["pool", "masks_only"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_scene_with_alpha_gradient(frame, pool):
    """dL/dalpha given (the ALPHA instantiations of the backward): colour, depth and alpha losses together."""
    from test_gpu_alpha import zero_channel
    orc = _orc()
    args = _scene(frame)
    W, H = FRAMES[frame]
    ref = orc.render_forward_cuda(*to_numpy_args(args))
    zref = orc.render_forward_cuda(*to_numpy_args(zero_channel(args)))
    rng = np.random.default_rng(12)
    gc = rng.standard_normal((1, H, W, 3)).astype(np.float32)
    gd = rng.standard_normal((1, H, W)).astype(np.float32)
    gA = rng.standard_normal((1, H, W)).astype(np.float32)
    g1 = orc.render_backward_cuda(ref, gc, gd)
    gcz = np.zeros_like(gc); gcz[..., 2] = gA
    g2 = orc.render_backward_cuda(zref, gcz, np.zeros_like(gd))
    dargs = to_dev(args)
    with _flags(0 if pool else _C.DM2_FLAG_NO_PAIR_POOL):
        with _C.alpha_output(True):
            out = _C.render_forward_cuda(*dargs)
        g = _C.render_backward_cuda(out[0], *dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(), out[7], out[8],
                                    out[9], out[3], out[4], out[5], out[6], dL_dout_alpha=torch.from_numpy(gA).cuda())
    assert np.array_equal(out[1].cpu().numpy().view(np.uint32), ref.color.view(np.uint32))
    for name, x in zip(GRAD_NAMES, g):
        want = g1[name] if name == "verts_color" else g1[name].astype(np.float64) + g2[name]
        assert rel_linf(x.cpu().numpy(), want) <= GRAD_TOL, name


# ---- 2. clamp_bary_uv on its boundaries ---------------------------------------------------------------------------------------
def _boundary_args(temp):
    """One face over the whole 16 x 16 frame whose world triangle is (0,0,2) (1,0,2) (0,1,2); the ray of pixel k starts at
    (u_k, v_k, 0) and runs along +z, so Moeller-Trumbore returns (u_k, v_k) exactly (every product is with 0 or 1)."""
    orc = _orc()
    W = H = 16
    vals = np.array([-0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0], dtype=np.float32)
    uu, vv = np.meshgrid(vals, vals, indexing="ij")
    u, v = np.tile(uu.reshape(-1), 4), np.tile(vv.reshape(-1), 4)
    u[192:] = np.float32(0.375); v[192:] = np.linspace(-1, 2, 64).astype(np.float32)         # (a last quarter in general position)
    u64, v64 = u.astype(np.float64), v.astype(np.float64)
    for on in (u64 == 0, v64 == 0, u64 == 1, v64 == 1, u64 + v64 == 1, v64 == u64 - 1, v64 == u64 + 1):
        assert on.sum() >= 3
    assert {_region(a, b, 0.0) for a, b in zip(u64, v64)} == set(range(7))
    tri = np.array([[(-4.5, -3.5), (40.5, -2.5), (-3.5, 41.5)], [(3.25, 2.5), (9.5, 4.25), (5.5, 11.75)]], dtype=np.float32)
    tri = np.asarray(orc.aa_tables(tri.copy(), np.float32, reorder=True)["verts"], dtype=np.float32).reshape(2, 3, 2)
    vimg = tri.reshape(1, 6, 2).copy()
    vimg[0, 4, 1] = np.nan                                                                  # the second face: a NaN vertex
    t = orc.aa_tables(vimg[0].reshape(2, 3, 2).copy(), np.float32, reorder=False)
    verts = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2], [0, 0, 3], [1, 0, 3], [0, 1, 3]], dtype=np.float32)
    ray_o = np.stack([u, v, np.zeros_like(u)], axis=-1).reshape(1, H, W, 3)
    ray_d = np.broadcast_to(np.array([0, 0, 1], np.float32), ray_o.shape).copy()
    rng = np.random.default_rng(5)
    T = torch.from_numpy
    ndc = np.concatenate([vimg[0] / 8 - 1, np.array([[-0.5]] * 3 + [[-0.25]] * 3)], axis=1).astype(np.float32)
    args = [T(rng.uniform(0, 1, 3).astype(np.float32)), torch.zeros((1, 2), dtype=torch.int32), W, H, T(verts),
            T(np.arange(6, dtype=np.int32).reshape(2, 3)), T(rng.uniform(0, 1, (6, 3)).astype(np.float32)),
            T(np.array([0.6, 0.5], np.float32)), T(ndc[None]), T(vimg), T(np.array([[0.9, 0.8]], np.float32)), float(temp)]
    for name in ("verts", "edges", "iszero", "recip", "normal"):
        args.append(T(np.ascontiguousarray(t[name]).reshape(1, 2, 3, 2)))
    args += [T(np.ascontiguousarray(t["normal_c"]).reshape(1, 2, 3)), 20, T(ray_o), T(ray_d)]
    return args


@pytest.mark.parametrize("route", ["pool", "masks_only", "point"])
def test_clamp_boundaries_through_the_op(route):
    args = _boundary_args(0.0 if route == "point" else 1.0)
    with _flags(_C.DM2_FLAG_NO_PAIR_POOL if route == "masks_only" else 0):
        res = run_both(args, seed=7)
        assert _C.last_forward_mode() == {"pool": _C.FWD_POOL, "masks_only": _C.FWD_MASKS, "point": _C.FWD_POINT}[route]
    check_forward(res, args)
    check_backward(res)
    assert np.abs(res["grads"][1]).max() > 0


# ---- 3. nothing moved -----------------------------------------------------------------------------------------------------------
def forward_five(args):
    """colour, depth, final_T, n_contrib, tri_cnt of one forward of the default route."""
    out = _C.render_forward_cuda(*to_dev(args))
    B, H, W = out[2].shape
    N, Tn = B * H * W, _C._tiles(B, W, H)
    fT = _C.debug_fetch(2, N, Tn, out[0], out[9], torch.float32, N).cpu().numpy()
    nc = _C.debug_fetch(4, N, Tn, out[0], out[9], torch.int32, N).cpu().numpy()
    return dict(color=out[1].cpu().numpy(), depth=out[2].cpu().numpy(), final_T=fT, n_contrib=nc, tri_cnt=out[5].cpu().numpy())


def golden_inputs(name):
    if name == "cfg1":
        import bench
        return bench.build_inputs("cfg1", torch.device("cuda", 0), 0, 1)[0]
    frame, classes = name.split("_")
    return build_scene(frame, classes == "classes")[0]


GOLDEN_CASES = ["16x16_single", "16x16_classes", "40x24_single", "40x24_classes", "cfg1"]


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_forward_outputs_bit_equal_to_recorded(name):
    g = {}                                                           # (cfg 1's colour is a file of its own: no file above 1 MiB)
    for f in [f"straightline_{name}.npz"] + (["straightline_cfg1_color.npz"] if name == "cfg1" else []):
        part = np.load(os.path.join(GOLDEN, f))
        assert len(str(part["library_commit"])) == 40
        g.update({k: part[k] for k in part.files})
    got = forward_five(golden_inputs(name))
    for k, a in got.items():
        want = g[k]
        assert a.dtype == want.dtype and a.shape == want.shape, k
        assert np.array_equal(a.view(np.uint32), want.view(np.uint32)), (k, int((a.view(np.uint32) != want.view(np.uint32)).sum()))
