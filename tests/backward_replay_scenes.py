"""Hand-built scenes for the backward's per-pixel replay (tests/test_gpu_backward_replay.py, tests/test_backward_replay_scenes.py).

Image space and world space coincide as in tests/test_gpu_straightline.py: world vertex = (x_img, y_img, z), the ray of pixel
(x, y) starts at (x + 0.5, y + 0.5, 0) and runs along +z, so a pair's (u, v) are the barycentrics of the pixel centre.  Face i
lies in front of face i + 1.  Every scene lives in an 8 x 8 pixel corner of one tile: at (5, 3) of the 16 x 16 frame, in the
partial tile at (32, 16) of the 40 x 24 frame (its larger faces reach into the neighbouring tiles).

``present_*`` assert from the oracle's forward state (n_contrib, final_T, final_prev_T, the tile lists) and from float64 geometry
that the situation a scene exists for is there; nothing of the library is involved."""
import numpy as np
import torch

FRAMES = {"16x16": (16, 16, 5, 3), "40x24": (40, 24, 32, 16)}       # W, H, and where the scene's 8 x 8 corner sits
BACKGROUND = (0.3, 0.6, 0.2)
T_EPS = 1e-4                                                         # the forward stops a pixel below it (forward.cu:391)


def _orc():
    from oracle import cpu as orc
    return orc


def _snap(tri):
    """Exact in float32 and never on a pixel line."""
    return np.round(np.asarray(tri, dtype=np.float64) * 64.0) / 64.0 + 1.0 / 256.0


def stack_tris(n, seed):
    """n small faces on the same pixels: under 3 px (n <= 30, one chunk holds them all) or ~4 px across."""
    rng = np.random.default_rng(seed)
    if n <= 30:                                                     # inside the pixels (1..3, 1..3): at most 9 pairs a face
        return [_snap(np.array([(1.2, 1.15), (3.85, 1.2), (1.25, 3.85)]) + rng.uniform(-0.1, 0.1, (3, 2))) for _ in range(n)]
    return [_snap(np.array([(1.2, 1.1), (5.9, 1.8), (2.3, 5.8)]) + rng.uniform(-0.3, 0.3, (3, 2))) for _ in range(n)]


def stack_scene(frame, n, temp=1.0):
    """-> (args, info).  Low opacities keep T alive through the whole stack."""
    W, H, ox, oy = FRAMES[frame]
    tris = [t + np.array([ox, oy], dtype=np.float64) for t in stack_tris(n, 100 + n)]
    rng = np.random.default_rng(200 + n)
    opac = rng.uniform(0.05, 0.2, n) if n <= 30 else rng.uniform(0.02, 0.06, n)
    return make_args(tris, opac, W, H, temp, seed=300 + n), dict(n=n, tile=_tile_of(frame))


# the opaque scene: faces 0..2 in front, 3 the opaque one, 4 hidden behind it, 5..14 behind it and beyond it
OPAQUE, HIDDEN, N_FRONT, N_BEHIND = 3, 4, 3, 10


def opaque_scene(frame, temp=1.0):
    W, H, ox, oy = FRAMES[frame]
    rng = np.random.default_rng(17)
    tris = [_snap(np.array([(0.8, 0.7), (3.4, 0.9), (1.0, 3.3)]) + rng.uniform(-0.1, 0.1, (3, 2))) for _ in range(N_FRONT)]
    tris.append(_snap([(0.5, 0.5), (7.5, 0.6), (0.6, 7.5)]))                       # opacity 1: covers pixels (1..5, 1..5), x + y <= 6, fully
    tris.append(_snap([(2.2, 1.3), (3.8, 1.4), (2.5, 2.7)]))                       # only on pixels the opaque face covers fully
    tris += [_snap(np.array([(-0.7, -0.6), (11.5, -0.5), (-0.6, 11.4)]) + rng.uniform(-0.3, 0.3, (3, 2))) for _ in range(N_BEHIND)]
    tris = [t + np.array([ox, oy], dtype=np.float64) for t in tris]
    opac = rng.uniform(0.2, 0.4, len(tris))
    opac[OPAQUE] = 1.0
    return make_args(tris, opac, W, H, temp, seed=41), dict(tile=_tile_of(frame))


# the threshold scene: the opaque scene's faces; 0..4 transparent, 5 and 6 take T to T_EPS exactly, 7..14 behind them
TH_A, TH_B = N_FRONT + 2, N_FRONT + 3
THRESHOLD_STEPS = (0, -1, 1)


def threshold_scene(frame, step=0, temp=1.0):
    """Pixels whose transmittance lands on T_EPS exactly (tests/test_gpu_composite.py::test_the_stop_is_strictly_below_T_EPS):
    1 - a = 8192 T_EPS and 1 - b = 2^-13 are exact in float32 and so is their product, and where the two large faces TH_A, TH_B
    cover a pixel fully their alphas are their opacities a and b to the bit.  T < T_EPS is false there: the face behind them
    still blends (T <= T_EPS would end the pixel one face early).  ``step``: 1 - a that many ulps away from 8192 T_EPS (-1:
    T one ulp below T_EPS, the pixel ends at TH_B; +1: it goes on)."""
    W, H, ox, oy = FRAMES[frame]
    f32 = np.float32
    x = f32(T_EPS) * f32(8192)
    if step:
        x = np.nextafter(x, f32(0) if step < 0 else f32(1))
    a, b = f32(1) - x, f32(1) - f32(2.0 ** -13)
    assert f32(1) - a == x
    assert (x * (f32(1) - b) == f32(T_EPS)) == (step == 0)
    rng = np.random.default_rng(17)
    tris = [_snap(np.array([(0.8, 0.7), (3.4, 0.9), (1.0, 3.3)]) + rng.uniform(-0.1, 0.1, (3, 2))) for _ in range(N_FRONT)]
    tris.append(_snap([(0.5, 0.5), (7.5, 0.6), (0.6, 7.5)]))
    tris.append(_snap([(2.2, 1.3), (3.8, 1.4), (2.5, 2.7)]))
    tris += [_snap(np.array([(-0.7, -0.6), (11.5, -0.5), (-0.6, 11.4)]) + rng.uniform(-0.3, 0.3, (3, 2))) for _ in range(N_BEHIND)]
    tris = [t + np.array([ox, oy], dtype=np.float64) for t in tris]          # (the opaque scene's faces, draw for draw)
    opac = rng.uniform(0.2, 0.4, len(tris)).astype(f32)
    opac[:TH_A] = 0.0                                                        # in front: alpha 0, T stays exactly 1
    opac[TH_A], opac[TH_B] = a, b
    return make_args(tris, opac, W, H, temp, seed=43), dict(tile=_tile_of(frame), step=step)


def present_threshold(args, ref, info):
    """-> the pixels of the tile that TH_A, TH_B and the face behind them cover fully: T behind TH_B is (1 - a)(1 - b) there,
    and n_contrib says on which side of the stop that fell."""
    W, H, nc, fT, fpT, lens = _state(args, ref)
    tris = _tris(args)
    tm = _tile_mask(info["tile"], W, H)
    full = _fully_inside(tris[TH_A], W, H) & _fully_inside(tris[TH_B], W, H) & _fully_inside(tris[TH_B + 1], W, H) & tm
    assert full.sum() >= 6, int(full.sum())
    op = args[7].numpy()
    T2 = (np.float32(1) - op[TH_A]) * (np.float32(1) - op[TH_B])
    if info["step"] < 0:
        assert T2 < np.float32(T_EPS) and (nc[full] == TH_B + 1).all() and (fT[full] == T2).all()
    else:
        assert (T2 == np.float32(T_EPS)) == (info["step"] == 0) and T2 >= np.float32(T_EPS)
        assert (nc[full] > TH_B + 1).all() and (fpT[full] <= T2).all()      # the stop did not fire at T == T_EPS
    return full


def _tile_of(frame):
    W, H, ox, oy = FRAMES[frame]
    return (oy // 16) * ((W + 15) // 16) + ox // 16


def make_args(tris, opac, W, H, temp, seed):
    """The 21 boundary arguments (CPU tensors) for image-space triangles in depth order (tests/test_gpu_straightline.py)."""
    orc = _orc()
    tri = np.stack(tris).astype(np.float32)
    t = orc.aa_tables(tri.copy(), np.float32, reorder=True)
    tri = np.asarray(t["verts"], dtype=np.float32).reshape(-1, 3, 2)      # table order = vertex order: the world faces never swap
    F = tri.shape[0]
    assert F <= 96
    rng = np.random.default_rng(seed)
    z = 1.0 + 0.01 * np.arange(F, dtype=np.float32)
    verts = np.concatenate([tri.reshape(-1, 2), np.repeat(z, 3)[:, None]], axis=1).astype(np.float32)
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    vimg = tri.reshape(1, -1, 2).copy()
    ndc = np.stack([vimg[0, :, 0] * 2 / W - 1, vimg[0, :, 1] * 2 / H - 1, np.repeat(-0.5 + 0.01 * np.arange(F), 3)], axis=1)
    t = orc.aa_tables(vimg[0].reshape(F, 3, 2).copy(), np.float32, reorder=True)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ray_o = np.stack([xs + 0.5, ys + 0.5, np.zeros_like(xs)], axis=-1)[None]
    ray_d = np.broadcast_to(np.array([0, 0, 1], np.float32), ray_o.shape).copy()
    T = torch.from_numpy
    args = [T(np.array(BACKGROUND, np.float32)), torch.zeros((1, 2), dtype=torch.int32), W, H, T(verts), T(faces),
            T(rng.uniform(0, 1, (3 * F, 3)).astype(np.float32)), T(np.asarray(opac, dtype=np.float32)),
            T(ndc[None].astype(np.float32)), T(vimg), T(rng.uniform(0.5, 1.0, (1, F)).astype(np.float32)), float(temp)]
    for name in ("verts", "edges", "iszero", "recip", "normal"):
        args.append(T(np.ascontiguousarray(t[name]).reshape(1, F, 3, 2)))
    args += [T(np.ascontiguousarray(t["normal_c"]).reshape(1, F, 3)), 20, T(ray_o), T(ray_d)]
    return args


# ---- what is there, from the oracle's forward state and float64 geometry ---------------------------------------------------------
def _centre_inside(tri, W, H):
    """(H, W) bool: pixel centres strictly inside the triangle (float64)."""
    tri = np.asarray(tri, dtype=np.float64)
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    s = []
    for i in range(3):
        a, b = tri[i], tri[(i + 1) % 3]
        s.append((b[0] - a[0]) * (ys - a[1]) - (b[1] - a[1]) * (xs - a[0]))
    s = np.stack(s)
    return (s > 0).all(axis=0) | (s < 0).all(axis=0)


def _fully_inside(tri, W, H):
    """(H, W) bool: pixels whose four corners are strictly inside the triangle."""
    tri = np.asarray(tri, dtype=np.float64)
    out = np.ones((H, W), dtype=bool)
    for cx, cy in ((0, 0), (1, 0), (1, 1), (0, 1)):
        out &= _centre_inside(tri - np.array([cx - 0.5, cy - 0.5]), W, H)
    return out


def _bbox_pixels(tri, W, H):
    tri = np.asarray(tri, dtype=np.float64)
    x0, x1 = max(0, int(np.floor(tri[:, 0].min()))), min(W, int(np.ceil(tri[:, 0].max())))
    y0, y1 = max(0, int(np.floor(tri[:, 1].min()))), min(H, int(np.ceil(tri[:, 1].max())))
    m = np.zeros((H, W), dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


def _tile_mask(tile, W, H):
    gx = (W + 15) // 16
    ty, tx = divmod(tile, gx)
    m = np.zeros((H, W), dtype=bool)
    m[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = True
    return m


def _tris(args):
    return args[9].numpy().reshape(-1, 3, 2).astype(np.float64)


def _state(args, ref):
    W, H = args[2], args[3]
    lens = (ref.binning.ranges[:, 1].astype(np.int64) - ref.binning.ranges[:, 0].astype(np.int64))
    return W, H, ref.n_contrib.reshape(H, W), ref.final_T.reshape(H, W), ref.final_prev_T.reshape(H, W), lens


def present_stack(args, ref, info):
    """Pixels that own one record of every face of the stack.  n <= 30: all pairs of the tile fit one chunk (<= 256), so such a
    pixel owns n records of that chunk.  n > 30: more entries than a chunk has candidates and more pairs than a chunk has lanes,
    and a pixel whose T is alive behind more than 30 entries."""
    W, H, nc, fT, _, lens = _state(args, ref)
    n, tile = info["n"], info["tile"]
    tris = _tris(args)
    tm = _tile_mask(tile, W, H)
    assert lens[tile] == n
    centres = sum(int((_centre_inside(t, W, H) & tm).sum()) for t in tris)          # every one of them blends (coverage > 0, region 0)
    touched = sum(int((_bbox_pixels(t, W, H) & tm).sum()) for t in tris)            # no pair outside a face's bounding box
    every = np.logical_and.reduce([_centre_inside(t, W, H) for t in tris]) & tm
    assert every.sum() >= 2, int(every.sum())
    assert (nc[every] == n).all() and (fT[every] > T_EPS).all() and (fT[every] < 1).all()
    if n <= 30:
        assert touched <= 256 and centres >= 3 * n, (centres, touched)
    else:
        assert centres > 256 and (nc[tm] > 30).any(), centres
    return every


def present_opaque(args, ref, info):
    """-> (pixels ended by the opaque face with faces in front, pixels whose only contributor it is, pixels that go on)."""
    W, H, nc, fT, fpT, lens = _state(args, ref)
    tile = info["tile"]
    tris = _tris(args)
    tm = _tile_mask(tile, W, H)
    full = _fully_inside(tris[OPAQUE], W, H) & tm                                   # coverage 1, region 0 -> alpha == 1
    assert lens[tile] == len(tris) == N_FRONT + 2 + N_BEHIND
    assert full.sum() >= 6 and (fT[full] == 0).all() and (nc[full] == OPAQUE + 1).all()
    assert (nc[full] < lens[tile]).all()                                            # entries behind the last contributor
    fronted = full & (fpT < 1)
    alone = full & (fpT == 1)
    assert fronted.sum() >= 1 and alone.sum() >= 1, (int(fronted.sum()), int(alone.sum()))
    return fronted, alone, full


def present_guard(args, ref, info):
    """A pixel that terminates early while others of its tile go on through the entries behind it; and a face behind the opaque
    one that no other pixel sees."""
    W, H, nc, fT, _, lens = _state(args, ref)
    _, _, full = present_opaque(args, ref, info)
    tile = info["tile"]
    tm = _tile_mask(tile, W, H)
    assert (nc[tm & ~full] == lens[tile]).any()                                     # neighbours reach the tile's last entry
    hidden = _bbox_pixels(_tris(args)[HIDDEN], W, H)
    assert hidden.any() and (hidden <= full).all()                                  # every pixel it touches ended in front of it
