"""Restatement of Renderer.rasterize(overlap=True) and Renderer.coverage(inside=...) for the tests (include/dm2_hip.h:
dm2_rasterize_run with overlap != 0, dm2_coverage's inside), in numpy on top of the restatements the tests already have.

Per pixel (x, y) of view b (of a window at patch_min, or the full frame) the candidates are ``window_ref.candidates``: the
pixel's tile list with the faces of existence 0 taken out.  A candidate f is listed iff
  (a) the oracle's clipper (``coverage_ref._overlaps``: ``orc_aa_overlap_f32`` on ``aa_tables(reorder=True)`` of
      verts_image[b, faces[f]]) reports no error and area != 0 for the pixel [X, X+1] x [Y, Y+1], (X, Y) = (x, y) + patch_min[b];
  (b) ``ray_tri32`` succeeds and ``rasterize_ref.off_plane32`` holds;
  (c) the slot's t >= 0,
with (uc, vc, code) = ``clamp32(u, v)``, bary = ((1 - uc) - vc, uc, vc), inside = (code == 0), and t = the intersection's t when
code == 0, else ``proj_t32``:

    b0 = (1 - uc) - vc;  d_k = dot(p_k - ro, rd);  t = ((b0 * d0 + uc * d1) + vc * d2) / dot(rd, rd)

in float32 in this order (dot = (x x + y y) + z z; numpy float32 arithmetic is IEEE and uncontracted, like the kernels).  The
listed candidates are ordered by (t, face id) -- the exhaustive selection, no early exit -- and the first L make the slots; empty
slots hold -1 (False in inside).

* ``evaluate`` / ``select`` -- the above; ``evaluate`` is what does not depend on L.
* ``grads64`` -- float64 torch autograd of (bary, t) w.r.t. verts over given lists, the float32 clamp codes held fixed.
* ``coverage32`` -- coverage with the inside mask: a non-empty slot with inside == 0 mixes as area * temperature.
* ``scene`` -- the scenes of the CPU and GPU tests (B = 2), ``staircase`` the scene of the equivalence with Renderer.forward,
  ``deferred32`` / ``forward32`` the two sides of that equivalence on the CPU.
"""
import numpy as np
import torch

import coverage_ref as cref
import rasterize_ref as rref
import window_ref as wref
from layer_composite_ref import _dot, clamp_code32, ray_tri32

f32 = np.float32
NO_ID = rref.NO_ID
TILE = rref.TILE


def _np(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


# ---- the per-slot formulas, float32 ------------------------------------------------------------------------------------------------
def clamp32(u, v):
    """clamp_bary_uv (dm2_device_math.h; auxiliary.h:292-329) on float32 arrays -> (uc, vc, code)."""
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    code = clamp_code32(u, v)
    one, half, zero = f32(1), f32(0.5), f32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        ue = ((one + u) - v) * half
        ve = ((one - u) + v) * half
    uc = np.select([code == 0, code == 1, code == 2, code == 3, code == 4, code == 5], [u, zero, one, zero, zero, u], ue).astype(f32)
    vc = np.select([code == 0, code == 1, code == 2, code == 3, code == 4, code == 5], [v, zero, zero, one, v, zero], ve).astype(f32)
    return uc, vc, code


def proj_t32(ro, rd, p0, p1, p2, uc, vc):
    """The t of a slot whose clamp code is not 0 (dm2_rasterize.hip rz_proj_t), float32, in the contract's order."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        b0 = (f32(1) - uc) - vc
        d0, d1, d2 = _dot(p0 - ro, rd), _dot(p1 - ro, rd), _dot(p2 - ro, rd)
        return (((b0 * d0 + uc * d1) + vc * d2) / _dot(rd, rd)).astype(f32)


# ---- listing ---------------------------------------------------------------------------------------------------------------------
def full_window(s):
    B = s["verts_ndc"].shape[0]
    return np.zeros((B, 2), np.int32), int(s["W"]), int(s["H"])


def evaluate(s, win=None, face_existence=None):
    """Every pixel's candidates with what the listing rule needs -> dict(shape (B, ph, pw), cand (N, J), listed (N, J) bool,
    t, uc, vc (N, J) float32, code (N, J) int32, area (N, J) float32 and err (N, J) int32: the clipper's (0 where it was not
    asked), pm)."""
    pm, pw, ph = full_window(s) if win is None else win
    pm = np.asarray(pm, np.int32)
    cand, _, _ = wref.candidates(s, pm, pw, ph, face_existence)
    B = s["verts_ndc"].shape[0]
    N, J = cand.shape
    vs, fc, vi = _np(s["verts"], f32), _np(s["faces"], np.int32), _np(s["verts_image"], f32)
    ro, rd = wref.rays(s, pm, pw, ph)
    ro, rd = ro.reshape(N, 1, 3), rd.reshape(N, 1, 3)
    have = cand >= 0
    cs = np.where(have, cand, 0)
    vid = fc[cs]
    p0, p1, p2 = vs[vid[..., 0]], vs[vid[..., 1]], vs[vid[..., 2]]
    ok, t0, u, v = ray_tri32(ro, rd, p0, p1, p2)
    uc, vc, code = clamp32(u, v)
    t = np.where(code == 0, t0, proj_t32(ro, rd, p0, p1, p2, uc, vc)).astype(f32)
    with np.errstate(invalid="ignore"):
        ray = have & ok & rref.off_plane32(rd, p0, p1, p2) & (t >= 0)
    # the clipper is asked only where the pixel's square comes within a pixel of the triangle's bbox (float64, with that margin:
    # a pair further apart has no overlap whatever the rounding)
    b, y, x = np.meshgrid(np.arange(B), np.arange(ph), np.arange(pw), indexing="ij")
    X = (x + pm[:, 0][:, None, None]).reshape(N, 1)
    Y = (y + pm[:, 1][:, None, None]).reshape(N, 1)
    bb = b.reshape(N, 1)
    tri = vi[bb[..., None], vid].astype(np.float64)                              # (N, J, 3, 2)
    with np.errstate(invalid="ignore"):
        near = ~((tri[..., 0].max(-1) < X - 1) | (tri[..., 0].min(-1) > X + 2) | (tri[..., 1].max(-1) < Y - 1) | (tri[..., 1].min(-1) > Y + 2))
    ask = ray & near
    area = np.zeros((N, J), f32)
    err = np.zeros((N, J), np.int32)
    if ask.any():
        pi, ji = np.nonzero(ask)
        keys = np.stack([bb[pi, 0], cand[pi, ji], Y[pi, 0], X[pi, 0]], 1).astype(np.int64)
        uniq, inv = np.unique(keys, axis=0, return_inverse=True)
        got = cref._overlaps(vi, fc, uniq)
        vals = [got[k] for k in map(tuple, uniq.tolist())]
        inv = inv.reshape(-1)
        area[pi, ji] = np.array([a for a, _, _ in vals], f32)[inv]
        err[pi, ji] = np.array([c for _, _, c in vals], np.int32)[inv]
    listed = ask & (err == 0) & (area != 0)
    return dict(shape=(B, ph, pw), cand=cand, listed=listed, t=t, uc=uc, vc=vc, code=code, area=area, err=err, pm=pm)


def select(x, num_layers):
    """The first L listed candidates in (t, id) order -> dict(layers (B,H,W,L) int32, cnt (B,H,W) int32, bary (B,H,W,L,3) float32,
    t (B,H,W,L) float32, inside (B,H,W,L) bool, area (B,H,W,L) float32: the listed slot's overlap, for the tests)."""
    L = int(num_layers)
    B, H, W = x["shape"]
    N = B * H * W
    cand, listed = x["cand"], x["listed"]
    J = cand.shape[1]
    kt = np.where(listed, x["t"], np.inf)
    kid = np.where(listed, cand, NO_ID)
    order = np.lexsort((kid, kt), axis=-1)[:, :L] if J else np.zeros((N, 0), np.int64)
    order = np.pad(order, ((0, 0), (0, L - order.shape[1])), constant_values=0)
    nh = np.minimum(listed.sum(1), L)
    have = np.arange(L)[None] < nh[:, None]
    s = np.where(have, order, 0)
    take = (lambda a, fill: np.where(have, np.take_along_axis(a, s, 1), fill)) if J else (lambda a, fill: np.full(have.shape, fill, a.dtype))
    ids = take(cand, -1).astype(np.int32)
    uc, vc = take(x["uc"], f32(0)).astype(f32), take(x["vc"], f32(0)).astype(f32)
    b0 = np.where(have, (f32(1) - uc) - vc, f32(-1)).astype(f32)
    bary = np.stack([b0, np.where(have, uc, f32(-1)), np.where(have, vc, f32(-1))], -1).astype(f32)
    return dict(layers=ids.reshape(B, H, W, L), cnt=have.sum(1).astype(np.int32).reshape(B, H, W), bary=bary.reshape(B, H, W, L, 3),
                t=take(x["t"], f32(-1)).astype(f32).reshape(B, H, W, L), inside=(take(x["code"], 1) == 0).reshape(B, H, W, L),
                area=take(x["area"], f32(0)).astype(f32).reshape(B, H, W, L))


OUTS = ("layers", "cnt", "bary", "t", "inside")


# ---- gradients -------------------------------------------------------------------------------------------------------------------
def slot_codes(verts, faces, layers, ray_o, ray_d):
    """The float32 clamp code of every slot of ``layers`` (B,H,W,L) at the given rays (B,H,W,3); -1 in an empty slot."""
    vs, fc, rl = _np(verts, f32), _np(faces, np.int32), _np(layers, np.int64)
    m = (rl >= 0) & (rl < fc.shape[0])
    vid = fc[np.where(m, rl, 0)]
    ro, rd = _np(ray_o, f32)[..., None, :], _np(ray_d, f32)[..., None, :]
    _, _, u, v = ray_tri32(ro, rd, vs[vid[..., 0]], vs[vid[..., 1]], vs[vid[..., 2]])
    return np.where(m, clamp32(u, v)[2], -1)


def clamp64(u, v, code):
    """clamp_bary_uv's result per region in torch float64, the region ``code`` given."""
    code = torch.as_tensor(code)
    zero, one = torch.zeros_like(u), torch.ones_like(u)
    uc = torch.where(code == 0, u, torch.where(code == 2, one, torch.where(code == 5, u, torch.where(code == 6, (1 + u - v) * 0.5, zero))))
    vc = torch.where(code == 0, v, torch.where(code == 3, one, torch.where(code == 4, v, torch.where(code == 6, (1 - u + v) * 0.5, zero))))
    return uc, vc


def slot_values64(ro, rd, p0, p1, p2, code):
    """(bary (n,3), t (n,)) of the overlap mode in torch float64 for the given clamp codes (differentiable)."""
    t, u, v = rref.uvt64(ro, rd, p0, p1, p2)
    uc, vc = clamp64(u, v, code)
    b = torch.stack([1 - uc - vc, uc, vc], -1)
    d = torch.stack([((p - ro) * rd).sum(-1) for p in (p0, p1, p2)], -1)
    tp = (b * d).sum(-1) / (rd * rd).sum(-1)
    return b, torch.where(torch.as_tensor(code) == 0, t, tp)


def grads64(verts, faces, layers, ray_o, ray_d, g_bary, g_t, codes=None):
    """dL/dverts (P,3) float64 of L = sum over the listed slots (0 <= f < F) of g_bary . bary + g_t t, bary and t the overlap
    mode's in float64 at the float32 ray, with each slot's float32 clamp code (``slot_codes``) held fixed."""
    vs = torch.tensor(_np(verts, np.float64), requires_grad=True)
    fc = torch.as_tensor(_np(faces, np.int64))
    rl = _np(layers, np.int64)
    B, H, W, L = rl.shape
    m = (rl >= 0) & (rl < fc.shape[0])
    codes = slot_codes(verts, faces, rl, np.reshape(_np(ray_o, f32), (B, H, W, 3)), np.reshape(_np(ray_d, f32), (B, H, W, 3))) if codes is None else codes
    pix = np.nonzero(m)
    f = torch.as_tensor(rl[m])
    ro = torch.as_tensor(_np(ray_o, np.float64).reshape(B, H, W, 3)[pix[:3]])
    rd = torch.as_tensor(_np(ray_d, np.float64).reshape(B, H, W, 3)[pix[:3]])
    vid = fc[f]
    b, t = slot_values64(ro, rd, vs[vid[:, 0]], vs[vid[:, 1]], vs[vid[:, 2]], codes[m])
    gb = torch.as_tensor(_np(g_bary, np.float64)[m]) if g_bary is not None else torch.zeros((len(f), 3), dtype=torch.float64)
    gt = torch.as_tensor(_np(g_t, np.float64)[m]) if g_t is not None else torch.zeros(len(f), dtype=torch.float64)
    loss = ((gb * b).sum(-1) + gt * t).sum()
    if len(f):
        loss.backward()
    return vs.grad.numpy() if vs.grad is not None else np.zeros(tuple(vs.shape), np.float64)


# ---- coverage with the inside mask -----------------------------------------------------------------------------------------------
def coverage32(render_layers, inside, verts_image, faces, temperature, info=None):
    """``coverage_ref.coverage32`` with the mask: -> (cov (B,H,W,L) float32, info).  A non-empty slot with inside == 0 gets
    float32(0.0 * double(1 - temperature) + double(area * temperature)) = area * temperature where the clipper gives a non-zero
    area without error (0 at temperature 0); every other slot is coverage_ref's."""
    info = cref.coverage32(render_layers, verts_image, faces, temperature) if info is None else info
    t = f32(temperature)
    graze = ~info["empty"] & (np.asarray(inside) == 0)
    ok = info["partial"] | info["full"]
    if t == 0:
        return np.where(graze, f32(0), info["cov"]).astype(f32), info
    mixed = (np.float64(0.0) * np.float64(f32(1) - t) + (info["area"] * t).astype(f32).astype(np.float64)).astype(f32)
    return np.where(graze, np.where(ok, mixed, f32(0)), info["cov"]).astype(f32), info


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
W0, H0 = 52, 46            # 4 x 3 tiles, the last column 4 and the last row 14 pixels: partial tiles on both axes
SCENES = ("soup", "lattice", "aligned", "degenerate")
_SCENES = {}


def _soup(W, H, F, seed, views, dc, shared):
    from dmesh2_renderer_amd import scenes
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + seed, num_cams=max(views) + 1, depth_complexity=dc, shared_verts=shared)
    return sc, sc.verts.numpy().copy(), sc.faces.numpy().copy(), sc.mv.numpy()[views], sc.proj.numpy()[views]


def _finish(W, H, verts, faces, fe, mv, proj, **extra):
    from oracle import cpu as orc
    prep = orc.prepare_faces(verts, faces, mv, proj, W, H)
    ro, rd = orc.analytic_rays(mv, proj, W, H)
    return dict(W=W, H=H, verts=verts.astype(f32), faces=faces.astype(np.int32), fe=fe, verts_ndc=prep["verts_ndc"],
                verts_image=prep["verts_image"], ray_o=ro, ray_d=rd, mv=mv, proj=proj, **extra)


def scene(name):
    """The scenes of the overlap tests, B = 2, float32 numpy (projections and rays from the oracle, as in rasterize_ref.scene):
      soup        52 x 46, 260 welded triangles, ~8 deep, views [2, 0] of three cameras (permuted)
      lattice     tet_lattice(n=3) at 52 x 46, views [1, 0], its own existence flags
      aligned     tet_scenes "aligned" (65 x 49): vertices on pixel rays, projected edges along pixel rows and columns
      degenerate  a soup with zero-area faces and faces behind the camera or before its near plane, views [1, 1] (repeated)
      crowded     36 x 36, 4000 small triangles: more than 256 candidates in every tile of the window at (3, 2) (several LDS
                  chunks) and more than 512 distinct listed faces in its full tile (the backward table's overflow route)
      staircase   ``staircase()``"""
    if name in _SCENES:
        return _SCENES[name]
    from dmesh2_renderer_amd import scenes
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "aligned":
        s = wref.scene2("aligned")
    elif name == "staircase":
        s = staircase()
    elif name == "lattice":
        views = [1, 0]
        ts = scenes.tet_lattice(W0, H0, 3, seed=scenes.SEED_BASE + 91, num_cams=2)
        s = _finish(W0, H0, ts.verts.numpy(), ts.faces.numpy(), ts.faces_existence.numpy().astype(np.int32), ts.mv.numpy()[views],
                    ts.proj.numpy()[views])
    elif name == "crowded":
        _, verts, faces, mv, proj = _soup(36, 36, 4000, 93, [0, 1], 3.0, False)
        s = _finish(36, 36, verts, faces, (rng.uniform(size=len(faces)) < 0.9).astype(np.int32), mv, proj)
    else:
        views = [2, 0] if name == "soup" else [1, 1]
        F = 260 if name == "soup" else 150
        _, verts, faces, mv, proj = _soup(W0, H0, F, 90, views, 8.0 if name == "soup" else 4.0, name == "soup")
        if name == "degenerate":
            faces[::7, 2] = faces[::7, 1]                                         # zero area: a repeated vertex
            behind = np.arange(3, F, 11)
            vid = faces[behind].reshape(-1)
            verts[vid, 2] = 3.5 + rng.uniform(0, 1.5, len(vid)).astype(f32)       # behind the camera (it sits at z = 3)
            near = np.arange(5, F, 13)
            verts[faces[near].reshape(-1), 2] = 2.5                               # between the camera and its near plane
        s = _finish(W0, H0, verts, faces, (rng.uniform(size=len(faces)) < 0.7).astype(np.int32), mv, proj)
    _SCENES[name] = s
    return s


CROWDED_WINDOW = (np.array([[3, 2], [1, 4]], np.int32), 32, 32)      # unaligned origins, 2 x 2 full window tiles


_EVAL = {}


def evaluated(name, win=None, exist=False):
    """``evaluate`` of ``scene(name)``, cached (win: a key of window_ref.windows, "crowded" for CROWDED_WINDOW, or None)."""
    key = (name, win, bool(exist))
    if key not in _EVAL:
        s = scene(name)
        w = None if win is None else (CROWDED_WINDOW if win == "crowded" else wref.windows(s["W"], s["H"])[win])
        _EVAL[key] = evaluate(s, w, s["fe"] if exist else None)
    return _EVAL[key]


def window_of(name, win):
    s = scene(name)
    return full_window(s) if win is None else (CROWDED_WINDOW if win == "crowded" else wref.windows(s["W"], s["H"])[win])


# ---- the equivalence with Renderer.forward ----------------------------------------------------------------------------------------
STAIR_L = 12
STAIR_F = 40
STAIR_PATCH = (np.array([[5, 3], [9, 6]], np.int32), 37, 29)        # the unaligned patch of the equivalence test


def staircase():
    """A seeded "staircase soup": F triangles, each parallel to the image plane of its camera-0 view at its own view depth
    2.2 + 0.05 f (every vertex of face f at exactly that depth), image radius ~6 px, over a 52 x 46 frame; views [0, 0] so that
    both views see the faces parallel.  The depth step, 0.05, is large against what the ray parameter of a clamped point can
    differ from the plane's along a ray (the point lies within a pixel's half diagonal of the ray: < 0.03 in world units at
    these depths, times the sine of the ray's angle to the axis, < 0.45), so forward's tile-list order (by depth) and the (t, id)
    order agree at every pixel: tests/test_overlap_cpu.py asserts it, with no exception allowed."""
    from dmesh2_renderer_amd import scenes
    W, H, F = W0, H0, STAIR_F
    g = np.random.RandomState(4242)
    t, aspect = scenes.TAN_HALF_FOV, W / H
    cx, cy = g.uniform(4, W - 4, F), g.uniform(4, H - 4, F)
    th0 = g.uniform(0, 2 * np.pi, F)
    rad = 6.0 * g.uniform(0.6, 1.4, (F, 3))
    ang = th0[:, None] + np.arange(3)[None] * (2 * np.pi / 3)
    px, py = cx[:, None] + rad * np.cos(ang), cy[:, None] + rad * np.sin(ang)
    depth = (2.2 + 0.05 * g.permutation(F))[:, None] * np.ones((1, 3))          # (face id and depth order unrelated)
    xv = (px / W * 2 - 1) * depth * aspect * t
    yv = (py / H * 2 - 1) * depth * t
    verts = np.stack([xv, yv, scenes.CAM_DIST - depth], -1).reshape(3 * F, 3).astype(f32)
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    faces[1::2] = faces[1::2][:, [0, 2, 1]]                                      # both orientations
    mv, proj = scenes.camera(W, H)
    mv, proj = np.stack([mv.numpy()] * 2), np.stack([proj.numpy()] * 2)
    return _finish(W, H, verts, faces, np.ones(F, np.int32), mv, proj,
                   verts_color=g.uniform(0, 1, (3 * F, 3)).astype(f32), faces_opacity=g.uniform(0.2, 0.9, F).astype(f32),
                   faces_intense=g.uniform(0.75, 1.25, (2, F)).astype(f32), background=np.array([0.2, 0.5, 0.9], f32))


def forward_args(s, win, temperature):
    """The oracle's 21 arguments of Renderer.forward on scene ``s`` over the window, AA tables from verts_image."""
    from util import from_image_oracle_args
    pm, pw, ph = win
    ro, rd = wref.rays(s, pm, pw, ph)
    F = s["faces"].shape[0]
    B = s["verts_ndc"].shape[0]
    ph4, ph3 = np.zeros((B, F, 3, 2), f32), np.zeros((B, F, 3), f32)
    args = [s["background"], np.asarray(pm, np.int32), pw, ph, s["verts"], s["faces"], s["verts_color"], s["faces_opacity"],
            s["verts_ndc"], s["verts_image"], s["faces_intense"], float(temperature), ph4, ph4, ph4.astype(np.uint8), ph4, ph4, ph3, 20,
            ro, rd]
    return from_image_oracle_args(args)


def forward32(s, win, temperature):
    """The float32 oracle's Renderer.forward -> dict(color (B,H,W,3), depth_raw (B,H,W): NDC z with background 1, alpha (B,H,W)
    = 1 - final T, n_contrib, binning)."""
    from oracle import cpu as orc
    r = orc.render_forward_cuda(*forward_args(s, win, temperature))
    B, H, W = r.depth.shape
    return dict(color=r.color, depth_raw=r.depth, alpha=(f32(1) - r.final_T.reshape(B, H, W)).astype(f32), n_contrib=r.n_contrib.reshape(B, H, W),
                binning=r.binning)


def deferred32(s, sel, temperature, win=None):
    """The deferred path restated in float32 on the lists ``sel`` (``select``'s, or rasterize_ref's with inside all true):
    interpolate(verts_color) * faces_intense[b, id], interpolate of NDC z, coverage with the mask, composite with background
    (background, 1) -> dict(color, depth_raw, alpha)."""
    import composite_ref as cmp
    pm, pw, ph = full_window(s) if win is None else win
    rl, bary, inside = sel["layers"], sel["bary"], sel["inside"]
    B = rl.shape[0]
    have = rl >= 0
    vid = s["faces"][np.where(have, rl, 0)]                                       # (B,H,W,L,3)
    b0, b1, b2 = bary[..., 0:1], bary[..., 1:2], bary[..., 2:3]
    vc = s["verts_color"]
    col = ((b0 * vc[vid[..., 0]] + b1 * vc[vid[..., 1]]) + b2 * vc[vid[..., 2]]).astype(f32)
    col = (col * s["faces_intense"][np.arange(B)[:, None, None, None], np.where(have, rl, 0)][..., None]).astype(f32)
    z = s["verts_ndc"][..., 2]
    zb = z[np.arange(B)[:, None, None, None, None], vid]
    dep = ((b0[..., 0] * zb[..., 0] + b1[..., 0] * zb[..., 1]) + b2[..., 0] * zb[..., 2]).astype(f32)
    values = np.where(have[..., None], np.concatenate([col, dep[..., None]], -1), f32(0)).astype(f32)
    frame = wref.embed(rl, pm, s["W"], s["H"], -1)
    cov_f, _ = coverage32(frame, wref.embed(inside, pm, s["W"], s["H"], False), s["verts_image"], s["faces"], temperature)
    cov = wref.cut(cov_f, pm, pw, ph)
    alpha = (s["faces_opacity"][np.where(have, rl, 0)] * cov).astype(f32)
    out, final_T, _ = cmp.forward32(values, alpha, rl, np.concatenate([s["background"], [f32(1)]]).astype(f32))
    return dict(color=out[..., :3], depth_raw=out[..., 3], alpha=(f32(1) - final_T).astype(f32), cov=cov)


def list_order_agrees(s, x, win=None):
    """(N,) bool: at the pixel, the listed candidates taken in the tile list's order -- forward's: the binning by depth that
    ``Renderer.forward`` walks -- are in ascending (t, id) order."""
    from oracle import cpu as orc
    pm, pw, ph = full_window(s) if win is None else win
    B, P, F = s["verts_ndc"].shape[0], s["verts"].shape[0], s["faces"].shape[0]
    bn = orc.Binning(B, P, F, pw, ph, np.ascontiguousarray(pm, np.int32), s["faces"], s["verts_ndc"], s["verts_image"])   # forward's keys
    tl = wref.tile_lists(bn)
    gx, gy = (pw + TILE - 1) // TILE, (ph + TILE - 1) // TILE
    b, y, xx = np.meshgrid(np.arange(B), np.arange(ph), np.arange(pw), indexing="ij")
    fwd = tl[((b * gy + y // TILE) * gx + xx // TILE).reshape(-1)]               # (N, Jf) forward's list per pixel
    N = fwd.shape[0]
    # each listed candidate's (t, id) key, looked up by face id
    key_t = np.full((N, F), np.inf)
    pi, ji = np.nonzero(x["listed"])
    key_t[pi, x["cand"][pi, ji]] = x["t"][pi, ji]
    ft = np.where(fwd >= 0, np.take_along_axis(key_t, np.where(fwd >= 0, fwd, 0), 1), np.inf)    # t in forward's order, inf = not listed
    good = np.ones(N, bool)
    assert (np.isfinite(ft).sum(1) == x["listed"].sum(1)).all()                  # every listed candidate is in forward's list
    for n in range(N):
        m = np.isfinite(ft[n])
        tt, ii = ft[n][m], fwd[n][m]
        good[n] = all((tt[k] < tt[k + 1]) or (tt[k] == tt[k + 1] and ii[k] < ii[k + 1]) for k in range(len(tt) - 1))
    return good
