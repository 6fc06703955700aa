"""Phase B1's pair decode by start marks and phase C's straight-line blend (dm2_forward_queue.hip) on hand-built scenes of one
to four 16 x 16 tiles, colour, depth and tri_cnt held to the CPU oracle bit for bit.

Image space and world space coincide as in test_gpu_straightline.py (the ray of pixel (x, y) starts at (x + 0.5, y + 0.5, 0) and
runs along +z).  Tile 0 carries the condition a scene is named after; ``conditions`` counts every face's pixel rectangle in
numpy (the rule of face_pixel_rect, dm2_pairs.h) over the oracle's own tile lists and asserts that the scene reaches it before
anything is compared.  A second tile holds what steers the launcher's choice between the single-class and the by-class
instantiation: a few faces of many pixels or many faces of one pixel."""
import numpy as np
import pytest
import torch

from util import check_backward, check_forward, run_both, to_dev, to_numpy_args

from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

CHUNK, PAIRCAP, SURVCAP, TILE = 52, 768, 512, 16


def _orc():
    from oracle import cpu as orc
    return orc


# ---- faces (float64 image space; multiples of 1/64: exact in float32) ----------------------------------------------------------
def tiny(px, py):
    """Inside pixel (px, py): one pair."""
    return [(px + 0.25, py + 0.25), (px + 0.75, py + 0.375), (px + 0.375, py + 0.75)]


def box(x0, y0, w, h):
    """A right triangle whose rectangle is the w x h pixels from (x0, y0)."""
    return [(x0 + 0.25, y0 + 0.25), (x0 + w - 0.25, y0 + 0.25), (x0 + 0.25, y0 + h - 0.25)]


def cover(k=0):
    """Covers every pixel of the first row of tiles and far beyond."""
    return [(-4.5 - k, -3.5), (140.5 + k, -2.5 - k), (-3.5, 141.5 + k)]


def sliver(k):
    """A thin diagonal band across tile 0: the rectangle is the whole tile, few pixels survive the classification."""
    return [(0.25, 0.25 + k / 64.0), (15.75, 15.25 + k / 64.0), (15.75, 15.75)]


def _tile0(name):
    """-> (faces, opacity per face, indices of faces whose AA table gets NaN x coordinates)."""
    if name == "full_face":
        return [box(2, 3, 4, 5), cover(), box(9, 9, 3, 2)], [0.3, 0.2, 0.4], []
    if name == "paircap":
        return [sliver(k) for k in range(5)], [0.3] * 5, []
    if name == "survcap":
        return [cover(0), cover(1), cover(2)], [0.1, 0.15, 0.2], []
    if name == "straddle":                      # 36 pairs per face: offsets 0, 36, 72, 108, ...: rounds of 64 and Q = 128 are straddled
        return [box(2 * (k % 5), 9 * (k // 5), 6, 6) for k in range(9)], [0.25] * 9, []
    if name == "few_pairs":
        return [box(3, 4, 5, 4), tiny(8, 8), box(10, 1, 3, 6)], [0.3, 0.5, 0.2], []
    if name == "long_list":                     # 54 one- to four-pair faces, then opaque covers: every pixel ends at entry 55
        f = [tiny(k % 16, k // 16) if k % 3 else box(k % 14, 5 + k // 16, 2, 2) for k in range(54)]
        return f + [cover(k) for k in range(6)], [0.2] * 54 + [1.0] * 6, []
    if name == "empty_entries":                 # faces on the list with an empty rectangle: two in front, one inside, two behind
        f = [box(1, 1, 5, 5), box(2, 2, 5, 5)] + [box(k, 2 * k, 6, 3) for k in range(4)] + [box(4, 4, 7, 7)] + \
            [box(8, k, 3, 7) for k in range(5)] + [box(3, 3, 8, 8), box(5, 2, 6, 9)]
        return f, [0.3] * len(f), [0, 1, 6, len(f) - 2, len(f) - 1]
    raise KeyError(name)


SCENES = ["full_face", "paircap", "survcap", "straddle", "few_pairs", "long_list", "empty_entries"]
FRAME = {"full_face": (32, 16), "survcap": (32, 32)}                # (the others: 32 x 16, two tiles)


def build(name, route):
    orc = _orc()
    W, H = FRAME.get(name, (32, 16))
    faces, opac, nan_faces = _tile0(name)
    if route == "classes":                      # tile 1: twelve faces of 15 x 15 pixels
        extra = [[(16.25 + k / 64.0, 0.25), (31.75, 0.5 + k / 64.0), (16.5, 15.75)] for k in range(12)]
    else:                                       # tile 1: 240 faces of one pixel
        extra = [tiny(16 + k % 16, (k // 16) % 16) for k in range(240)]
    faces = faces + extra
    opac = np.array(list(opac) + [0.05] * len(extra), dtype=np.float32)
    tri = np.array(faces, dtype=np.float64).astype(np.float32)
    assert np.array_equal(tri.astype(np.float64), np.array(faces, dtype=np.float64))
    tri = np.asarray(orc.aa_tables(tri.copy(), np.float32, reorder=True)["verts"], dtype=np.float32).reshape(-1, 3, 2)
    F = tri.shape[0]
    rng = np.random.default_rng(41)
    z = 1.0 + 0.001 * np.arange(F, dtype=np.float32)
    verts = np.concatenate([tri.reshape(-1, 2), np.repeat(z, 3)[:, None]], axis=1).astype(np.float32)
    vimg = tri.reshape(1, -1, 2).copy()
    ndc = np.stack([vimg[0, :, 0] * 2 / W - 1, vimg[0, :, 1] * 2 / H - 1, np.repeat(-0.5 + 0.001 * np.arange(F), 3)], axis=1)
    table = tri.copy()
    table[nan_faces, :, 0] = np.nan             # every x of the face: fminf / fmaxf leave a NaN box -> an empty rectangle
    with np.errstate(invalid="ignore"):
        t = orc.aa_tables(table.copy(), np.float32, reorder=False)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ray_o = np.stack([xs + 0.5, ys + 0.5, np.zeros_like(xs)], axis=-1)[None]
    ray_d = np.broadcast_to(np.array([0, 0, 1], np.float32), ray_o.shape).copy()
    T = torch.from_numpy
    args = [T(rng.uniform(0, 1, 3).astype(np.float32)), torch.zeros((1, 2), dtype=torch.int32), W, H, T(verts),
            T(np.arange(3 * F, dtype=np.int32).reshape(F, 3)), T(rng.uniform(0, 1, (3 * F, 3)).astype(np.float32)), T(opac),
            T(ndc[None].astype(np.float32)), T(vimg), T(rng.uniform(0.5, 1.0, (1, F)).astype(np.float32)), 1.0]
    for key in ("verts", "edges", "iszero", "recip", "normal"):
        args.append(T(np.ascontiguousarray(t[key]).reshape(1, F, 3, 2)))
    args += [T(np.ascontiguousarray(t["normal_c"]).reshape(1, F, 3)), 20, T(ray_o), T(ray_d)]
    return args


# ---- the rectangles, in numpy ------------------------------------------------------------------------------------------------------
def rect_count(v, X0, Y0, W, H):
    """face_pixel_rect (dm2_pairs.h) for the AA table triangle v (3, 2) float32 in the tile at (X0, Y0): pairs, (x0, y0, w, h)."""
    with np.errstate(invalid="ignore"):
        bb = [np.fmin.reduce(v[:, 0]), np.fmax.reduce(v[:, 0]), np.fmin.reduce(v[:, 1]), np.fmax.reduce(v[:, 1])]
    if any(np.isnan(b) for b in bb):
        return 0, None
    x0 = max(0, int(np.clip(np.ceil(bb[0]) - 1 - X0, -1, 17))); x1 = min(min(TILE - 1, W - 1 - X0), int(np.clip(np.floor(bb[1]) - X0, -1, 17)))
    y0 = max(0, int(np.clip(np.ceil(bb[2]) - 1 - Y0, -1, 17))); y1 = min(min(TILE - 1, H - 1 - Y0), int(np.clip(np.floor(bb[3]) - Y0, -1, 17)))
    if x1 < x0 or y1 < y0:
        return 0, None
    return (x1 - x0 + 1) * (y1 - y0 + 1), (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def pixels_fully_inside(v, rect, X0, Y0):
    """Pixels of the rectangle whose four corners lie strictly inside the triangle (float64): they survive any classification."""
    v = v.astype(np.float64)
    a, b = v, np.roll(v, -1, axis=0)
    x0, y0, w, h = rect
    n = 0
    for y in range(Y0 + y0, Y0 + y0 + h):
        for x in range(X0 + x0, X0 + x0 + w):
            s = [(b[:, 0] - a[:, 0]) * (cy - a[:, 1]) - (b[:, 1] - a[:, 1]) * (cx - a[:, 0]) for cx in (x, x + 1) for cy in (y, y + 1)]
            s = np.array(s)
            n += bool((s > 0).all() or (s < 0).all())
    return n


def conditions(args, ref):
    """What the first chunk of tile 0 reaches, from the oracle's list of the tile and the rectangles alone."""
    W, H = args[2], args[3]
    table = args[12].numpy()[0]
    lo, hi = [int(x) for x in ref.binning.ranges[0]]
    flist = ref.binning.face_list[lo:hi].astype(np.int64)
    assert flist.max() < table.shape[0]
    rc = [rect_count(table[f], 0, 0, W, H) for f in flist]
    cnt = np.array([c for c, _ in rc], dtype=np.int64)
    first = cnt[:CHUNK]
    off = np.concatenate([[0], np.cumsum(first)])
    got = set()
    if (cnt == 256).any(): got.add("full_face")
    if off[-1] > PAIRCAP: got.add("paircap")
    inside = sum(pixels_fully_inside(table[f], r, 0, 0) for f, (c, r) in zip(flist[:CHUNK], rc) if c)
    if off[-1] <= PAIRCAP and inside > SURVCAP: got.add("survcap")
    if 0 < off[-1] < 64: got.add("few_pairs")
    if off[-1] <= PAIRCAP:                      # (no cut 1: the waves' ranges follow from the total)
        Q = (((off[-1] + 3) >> 2) + 63) & ~63
        wave = {k for k in (Q, 2 * Q, 3 * Q) if k < off[-1]}
        rounds = {k for k in range(64, off[-1], 64)} - wave
        inner = lambda ks: any(off[j] < k < off[j + 1] for k in ks for j in range(len(first)))
        if inner(wave) and inner(rounds): got.add("straddle")
    if len(cnt) > CHUNK and off[-1] <= SURVCAP:  # (neither cut: the second chunk starts at entry 52)
        tile0 = ref.n_contrib.reshape(H, W)[:TILE, :TILE]
        if CHUNK < tile0.max() < len(cnt): got.add("long_list")
    if len(first) >= 5 and first[0] == 0 and first[1] == 0 and first[-1] == 0 and first[-2] == 0 and (first[2:-2] == 0).any() \
            and (first > 0).sum() >= 3:
        got.add("empty_entries")
    return got


_RUNS = {}


def _run(name, route):
    """One forward (+ backward) of the op and of the oracle per scene and route, shared by the tests below."""
    if (name, route) not in _RUNS:
        args = build(name, route)
        res = run_both(args, seed=11)
        res["classes"] = _C.last_pair_bound() >= 32 * res["out"][0]
        res["mode"] = _C.last_forward_mode()
        _RUNS[name, route] = (args, res)
    return _RUNS[name, route]


@pytest.mark.parametrize("route", ["single", "classes"])
@pytest.mark.parametrize("name", SCENES)
def test_scene_reaches_its_condition_and_matches_the_oracle(name, route):
    args, res = _run(name, route)
    assert name in conditions(args, res["ref"]), conditions(args, res["ref"])
    assert res["mode"] == _C.FWD_POOL
    assert res["classes"] == (route == "classes")
    check_forward(res, args)                    # colour, depth, tri_cnt, final_T, n_contrib: bit for bit


@pytest.mark.parametrize("route", ["single", "classes"])
@pytest.mark.parametrize("name", ["straddle", "survcap"])
def test_backward_behind_it(name, route):
    """The backward reads the forward's masks and pair pool: gradients at the suite's tolerance show both are intact."""
    args, res = _run(name, route)
    check_backward(res)
    assert np.abs(res["grads"][1]).max() > 0


@pytest.mark.parametrize("route", ["single", "classes"])
@pytest.mark.parametrize("name", SCENES)
def test_scene_with_face_weights(name, route):
    """The WEIGHTS instantiations: the ten outputs as without the weights, the weights as the oracle's."""
    from test_gpu_face_weights import check_weights, oracle_weights
    args, res = _run(name, route)
    want, _ = oracle_weights(to_numpy_args(args))
    with _C.face_weights_output(True):
        out = _C.render_forward_cuda(*to_dev(args))
    assert (_C.last_pair_bound() >= 32 * out[0]) == (route == "classes")
    check_forward(dict(out=out[:10], ref=res["ref"]), args)
    check_weights(out[10], want, min_nonzero=3)
