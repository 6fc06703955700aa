"""Restatement of Renderer.coverage's contract (include/dm2_hip.h: dm2_coverage) for the tests, in numpy on top of the CPU
oracle's ``aa_tables`` / ``aa_overlap`` (oracle/cpu.py).

Per slot (b, y, x, l) with id f:
  empty           f outside [0, F), or faces[f] names a vertex outside [0, P): cov = 0, no gradient;
  temperature 0   cov = 1 in every non-empty slot, no clip, no gradient;
  otherwise       the triangle verts_image[b, faces[f]], CCW-reordered, its six tables from ``aa_tables(reorder=True)``, the pixel
                  [x, x+1] x [y, y+1], area and Jacobian from ``aa_overlap`` in float32; a clipper error or area == 0: cov = 0 and no
                  gradient; else cov = float32(1.0 * double(1 - temperature) + double(area * temperature)).

* ``coverage32`` -- cov plus the per-slot masks (empty / error / zero / partial / full) and the oracle's per-slot Jacobians.
* ``grad_image64`` -- dL/dverts_image (B,P,2) in float64: the float32 Jacobians times g_cov * temperature, scattered through the
  undone reorder (corner 0 is the face's vertex 0; corners 1 and 2 are its vertices 2 and 1 where the reorder swapped them): the
  twin of ``util.scatter_aa_grad_to_verts`` for per-slot Jacobians.
* the cases the CPU and GPU tests share, built once per process.  The oracle is called once per distinct (view, face, pixel).
"""
import os

import numpy as np

import rasterize_ref as rref

f32 = np.float32
TILE = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEMPERATURES = (1.0, 0.5, 0.0)


def _np(x, dtype):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def empty_slots(render_layers, faces, P):
    """(B,H,W,L) bool: the id is outside [0, F) or its face names a vertex outside [0, P)."""
    rl, fc = np.asarray(render_layers), np.asarray(faces).astype(np.int64).reshape(-1, 3)
    F = fc.shape[0]
    out = (rl < 0) | (rl >= F)
    if F:
        bad_face = ((fc < 0) | (fc >= P)).any(1)
        out = out | bad_face[np.where(out, 0, rl)]
    return out


def swapped(verts_image, faces):
    """(B,F) bool: the CCW reorder swaps corners 1 and 2 (pyrenderer.py:521-535, float32 as ``aa_tables`` evaluates it).  Faces
    with a vertex outside the table: False."""
    vi, fc = _np(verts_image, f32), _np(faces, np.int64).reshape(-1, 3)
    P = vi.shape[1]
    ok = ((fc >= 0) & (fc < P)).all(1)
    fs = np.where(ok[:, None], fc, 0)
    p0, p1, p2 = vi[:, fs[:, 0]], vi[:, fs[:, 1]], vi[:, fs[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        area = f32(0.5) * ((p1[..., 0] - p0[..., 0]) * (p2[..., 1] - p0[..., 1]) - (p2[..., 0] - p0[..., 0]) * (p1[..., 1] - p0[..., 1]))
        return (area < 0) & ok[None]


_PAIRS = {}        # (bytes of verts_image, bytes of faces) -> {(b, f, y, x): (area, J (3,2) float32, code)}


def _overlaps(vi, fc, keys):
    """The oracle's (area, Jacobian, code) of the distinct (b, f, y, x) rows of ``keys``; remembered per (verts_image, faces)."""
    from oracle import cpu as orc
    cache = _PAIRS.setdefault((vi.tobytes(), fc.tobytes()), {})
    todo = [k for k in map(tuple, keys.tolist()) if k not in cache]
    if todo:
        faces_used = sorted({(b, f) for b, f, _, _ in todo})
        row = {bf: i for i, bf in enumerate(faces_used)}
        tri = np.stack([vi[b, fc[f]] for b, f in faces_used])                       # (n, 3, 2)
        with np.errstate(all="ignore"):
            t = orc.aa_tables(tri, f32, reorder=True)
        # orc.aa_overlap's call, with the tables converted once instead of once per pair
        import ctypes
        fn = orc.lib().orc_aa_overlap_f32
        fn.restype = ctypes.c_int
        tabs = [np.ascontiguousarray(t[k], dt) for k, dt in (("verts", f32), ("edges", f32), ("iszero", np.uint8), ("recip", f32),
                                                             ("normal", f32), ("normal_c", f32))]
        base = [(a.ctypes.data, a.strides[0]) for a in tabs]
        area, J = np.zeros(1, f32), np.zeros((3, 2), f32)
        pa, pj = ctypes.c_void_p(area.ctypes.data), ctypes.c_void_p(J.ctypes.data)
        for b, f, y, x in todo:
            i = row[(b, f)]
            code = fn(*(ctypes.c_void_p(p0 + i * st) for p0, st in base), ctypes.c_float(x), ctypes.c_float(y), pa, pj)
            cache[(b, f, y, x)] = (f32(area[0]), J.copy(), int(code))
    return cache


def coverage32(render_layers, verts_image, faces, temperature):
    """-> dict(cov (B,H,W,L) float32, empty / error / zero / partial / full (B,H,W,L) bool, J (B,H,W,L,3,2) float32: the oracle's
    d(area)/d(reordered corners), zero wherever no gradient flows)."""
    rl, vi, fc = _np(render_layers, np.int32), _np(verts_image, f32), _np(faces, np.int32).reshape(-1, 3)
    if not (0.0 <= float(temperature) <= 1.0):
        raise ValueError("temperature must be in the range [0, 1]")
    t = f32(temperature)
    B, H, W, L = rl.shape
    empty = empty_slots(rl, fc, vi.shape[1])
    area = np.zeros(rl.shape, f32)
    code = np.zeros(rl.shape, np.int32)
    J = np.zeros(rl.shape + (3, 2), f32)
    live = np.argwhere(~empty)                                                      # rows (b, y, x, l)
    if len(live):
        keys = np.stack([live[:, 0], rl[~empty].astype(np.int64), live[:, 1], live[:, 2]], 1)
        uniq, inv = np.unique(keys, axis=0, return_inverse=True)
        got = _overlaps(vi, fc, uniq)
        vals = [got[k] for k in map(tuple, uniq.tolist())]
        inv = inv.reshape(-1)
        area[~empty] = np.array([v[0] for v in vals], f32)[inv]
        J[~empty] = np.stack([v[1] for v in vals])[inv]
        code[~empty] = np.array([v[2] for v in vals], np.int32)[inv]
    error = ~empty & (code != 0)
    zero = ~empty & ~error & (area == 0)
    full = ~empty & ~error & (area == 1)
    partial = ~empty & ~error & ~zero & ~full
    ok = partial | full
    if t == 0:
        cov = np.where(empty, f32(0), f32(1)).astype(f32)
        J = np.zeros_like(J)
    else:
        mixed = (np.float64(f32(1) - t) + (area * t).astype(f32).astype(np.float64)).astype(f32)      # forward.cu:375-378, a hit
        cov = np.where(ok, mixed, f32(0)).astype(f32)
        J = np.where(ok[..., None, None], J, f32(0)).astype(f32)       # (as the clipper returns it: zero at full cover, not where a
                                                                       # clipped polygon's area merely rounds to 1)
    return dict(cov=cov, empty=empty, error=error, zero=zero, partial=partial, full=full, J=J, area=area)


def grad_image64(render_layers, verts_image, faces, temperature, g_cov, info=None):
    """dL/dverts_image (B,P,2) float64 for upstream g_cov (B,H,W,L)."""
    rl, vi, fc = _np(render_layers, np.int32), _np(verts_image, f32), _np(faces, np.int64).reshape(-1, 3)
    info = coverage32(rl, vi, fc, temperature) if info is None else info
    B, P = vi.shape[0], vi.shape[1]
    out = np.zeros((B, P, 2), np.float64)
    m = (info["partial"] | info["full"]) if float(temperature) > 0 else np.zeros(rl.shape, bool)
    if not m.any():
        return out
    g = np.asarray(g_cov, dtype=np.float64)[m] * np.float64(f32(temperature))
    Jm = info["J"][m].astype(np.float64) * g[:, None, None]                          # (n, 3, 2)
    b = np.argwhere(m)[:, 0]
    f = rl[m].astype(np.int64)
    sw = swapped(vi, fc)[b, f]
    idx = fc[f].copy()                                                              # corner k -> vertex
    idx[:, 1] = np.where(sw, fc[f, 2], fc[f, 1])
    idx[:, 2] = np.where(sw, fc[f, 1], fc[f, 2])
    np.add.at(out, (np.repeat(b, 3), idx.reshape(-1)), Jm.reshape(-1, 2))
    return out


def upstream(shape, seed):
    """A random upstream gradient with exact zeros planted in a tenth of the slots."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(shape, dtype=f32)
    g[rng.uniform(size=shape) < 0.1] = 0
    return g


# ---- cases ---------------------------------------------------------------------------------------------------------------------
SCENE_LS = {"soup": (4,), "lattice": (1, 3, 8), "degenerate": (1, 3, 8), "no_faces": (3,)}
SCENE_LS.update(aligned=(4,), flat=(4,), duplicates=(4,))      # tet scenes (rasterize_ref.tet_case): axis-parallel projected
                                                                # edges and vertices on pixel centres; faces listed twice
SCENE_CASES = [(name, L) for name in rref.SCENES + ("aligned", "flat", "duplicates") for L in SCENE_LS[name]]
FIXTURE_CASES = [(name, key) for name in ("aa_pairs", "aa_error_pairs") for key in ("tri_in", "t_verts")]
REWOUND = ("soup", "degenerate")     # every face of these generators projects counter-clockwise: every other one is rewound here,
                                     # so that the lists hold both orientations and the reorder's swap is exercised on them too
_CASES, _INTERSECT = {}, {}


def _finish(c, seed):
    c["g"] = upstream(c["render_layers"].shape, seed)
    c["info"] = {t: coverage32(c["render_layers"], c["verts_image"], c["faces"], t) for t in TEMPERATURES}
    return c


def scene_case(name, L):
    """``rasterize_ref.scene(name)`` (REWOUND: vertices 1 and 2 of every other face exchanged) with ``rasterize32``'s lists at L
    layers -> dict(render_layers, verts_image, faces, W, H, g,
    info {temperature: coverage32})."""
    key = ("scene", name, L)
    if key not in _CASES and name in rref.TET_CASES:
        s = rref.tet_case(name)
        ras = rref.select(rref.tet_intersect(name), L)
        _CASES[key] = _finish(dict(render_layers=ras["layers"], verts_image=s["verts_image"], faces=s["faces"], W=s["W"], H=s["H"]),
                              sum(map(ord, name)) + L)
    if key not in _CASES:
        s = dict(rref.scene(name))
        if name in REWOUND:
            s["faces"] = s["faces"].copy()
            s["faces"][1::2] = s["faces"][1::2][:, [0, 2, 1]]
        if name not in _INTERSECT:
            _INTERSECT[name] = rref.intersect(s["W"], s["H"], s["verts"], s["faces"], None, s["verts_ndc"], s["verts_image"],
                                              s["ray_o"], s["ray_d"])
        ras = rref.select(_INTERSECT[name], L)
        _CASES[key] = _finish(dict(render_layers=ras["layers"], verts_image=s["verts_image"], faces=s["faces"], W=s["W"], H=s["H"]),
                              sum(map(ord, name)) + L)
    return _CASES[key]


def fixture_case(name, key):
    """The pairs of tests/golden/<name>.npz as one view: verts_image = ``key`` (tri_in or t_verts) reshaped to (1, 3n, 2), faces =
    arange(3n).reshape(n, 3), each pair listed at its pixmin, pairs that share a pixel in successive slots (``slot`` (n, 3) = y, x,
    l of pair i).  Behind the pairs: two faces that name a vertex outside the table, listed in free slots, and ids outside [0, F)."""
    ck = ("fixture", name, key)
    if ck not in _CASES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        n = len(g["pixmin"])
        side = 20 if name == "aa_pairs" else 60
        pm = g["pixmin"].astype(np.int64)
        assert (pm >= 0).all() and (pm < side).all()
        slot = np.zeros((n, 3), np.int64)
        fill = {}
        for i, (x, y) in enumerate(pm.tolist()):
            slot[i] = (y, x, fill.get((y, x), 0))
            fill[(y, x)] = slot[i, 2] + 1
        L = max(fill.values())
        rl = np.full((1, side, side, L), -1, np.int32)
        rl[0, slot[:, 0], slot[:, 1], slot[:, 2]] = np.arange(n)
        faces = np.concatenate([np.arange(3 * n).reshape(n, 3), [[0, 1, 3 * n], [-1, 4, 5]]]).astype(np.int32)
        free = np.argwhere(rl[0, ..., L - 1] < 0)
        outside = [n, n + 1, n + 2, -7, 2 ** 31 - 1, -2 ** 31]                      # two bad faces, then ids outside [0, F)
        for j, (y, x) in enumerate(free[:len(outside) * 3].tolist()):
            rl[0, y, x, L - 1] = outside[j % len(outside)]
        c = dict(render_layers=rl, verts_image=g[key].reshape(1, 3 * n, 2).astype(f32), faces=faces, W=side, H=side, slot=slot,
                 golden={k: g[k] for k in ("area_analytic", "msg_analytic", "err_analytic")})
        _CASES[ck] = _finish(c, n)
    return _CASES[ck]


def overflow_case():
    """One 16 x 16 tile, L = 4, 1024 distinct small triangles of either orientation, each inside or across its own pixel: more
    faces with a non-zero Jacobian in one block than its table has slots."""
    ck = ("overflow",)
    if ck not in _CASES:
        rng = np.random.default_rng(1024)
        L, n = 4, TILE * TILE * 4
        ys, xs, ls = np.meshgrid(np.arange(TILE), np.arange(TILE), np.arange(L), indexing="ij")
        centre = np.stack([xs, ys], -1).reshape(n, 1, 2) + rng.uniform(0.2, 0.8, (n, 1, 2))
        ang = rng.uniform(0, 2 * np.pi, (n, 1)) + np.arange(3) * 2 * np.pi / 3 + rng.uniform(-0.4, 0.4, (n, 3))
        rad = rng.uniform(0.15, 0.9, (n, 3))
        tri = centre + rad[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)
        tri[::2] = tri[::2, ::-1]                                                   # every other one clockwise
        faces = rng.permutation(3 * n).reshape(n, 3).astype(np.int32)
        vi = np.zeros((1, 3 * n, 2), f32)
        rl = rng.permutation(n).astype(np.int32)                                    # (face ids in no order of the pixels)
        vi[0, faces[rl].reshape(-1)] = tri.reshape(-1, 2).astype(f32)               # slot i lists face rl[i]: triangle i
        _CASES[ck] = _finish(dict(render_layers=rl.reshape(1, TILE, TILE, L), verts_image=vi, faces=faces, W=TILE, H=TILE), 7)
    return _CASES[ck]


def all_cases():
    """[(label, case)] of every shared case."""
    return ([(f"{n}-L{L}", scene_case(n, L)) for n, L in SCENE_CASES] + [(f"{n}-{k}", fixture_case(n, k)) for n, k in FIXTURE_CASES]
            + [("overflow", overflow_case())])


def area64(tri, pixmin):
    """Overlap area of triangle ``tri`` (3,2) with the pixel at ``pixmin`` in float64, tables rebuilt (reorder included):
    ``orc_aa_overlap_f64``.  -> (area, code)."""
    from oracle import cpu as orc
    with np.errstate(divide="ignore"):
        t = orc.aa_tables(np.asarray(tri, np.float64)[None], np.float64, reorder=True)
    area, _, code = orc.aa_overlap(t, 0, np.asarray(pixmin, np.float64), np.float64)
    return area, code
