"""Restatement of Renderer.rasterize's contract (include/dm2_hip.h: dm2_rasterize_run) for the tests.

* ``candidates`` -- each pixel's tile list from the oracle's own binning (``oracle.cpu.Binning(..., key_min_depth=True)``:
  the plan's bbox bins and depth cull, lists in min-depth order), with the faces of existence 0 taken out.
* ``rasterize32`` -- float32 Moeller-Trumbore in the device's operation order (``layer_composite_ref.ray_tri32``; numpy float32
  is IEEE and uncontracted like the kernels built with -ffp-contract=off), the hit test with its off-plane rule
  (``off_plane32``; ``rule=False`` gives the test without it), the (t, face id) order, the first L hits.  ``early_exit=True`` walks each pixel's list the way the kernel does instead -- passes of 16, each stopping at the
  first face whose min depth lies beyond the largest max depth of a full set of held hits -- so that a test can show the stop
  changes nothing; the contract is the result without it.
* ``grads64`` -- float64 torch autograd of (bary, t) w.r.t. verts over given (pixel, face) pairs.
* ``tet_case`` / ``tet_intersect`` -- the scenes of tests/tet_scenes.py as rasterize inputs; ``tie_pairs``, ``edge_hits``,
  ``rule_removed`` count what they reach.
* ``unsound64`` / ``clear_hits64`` / ``missing64`` -- a float64 brute force over all faces that reads nothing from the binning:
  no listed hit is wrong, no clear hit is missing.
"""
import numpy as np
import torch

from layer_composite_ref import _cross, _dot, ray_tri32

f32 = np.float32
PLANE_COS2 = f32(2.5e-7)    # dm2_rasterize.hip RZ_PLANE_COS2: the hit rule's bound on cos^2 of the angle (ray, face normal)
TILE = 16
PASS = 16                   # the kernel's longest register list
NO_ID = np.iinfo(np.int32).max


def _np(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def candidates(width, height, faces, face_existence, verts_ndc, verts_image):
    """-> (cand (N, J) int64 face ids of each pixel's tile list in list order, existing faces first, -1 = none; min_d, max_d
    (N, J) float32 of those faces), N = B*H*W pixels in (b, y, x) order."""
    from oracle import cpu as orc
    ndc, img, fc = _np(verts_ndc, f32), _np(verts_image, f32), _np(faces, np.int32)
    B, P, F = ndc.shape[0], ndc.shape[1], fc.shape[0]
    W, H = int(width), int(height)
    N = B * H * W
    if F == 0 or N == 0:
        z = np.zeros((N, 0), f32)
        return np.zeros((N, 0), np.int64), z, z
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    bn = orc.Binning(B, P, F, W, H, np.zeros((B, 2), np.int32), fc, ndc, img, key_min_depth=True)
    ranges = bn.ranges.astype(np.int64)
    lens = ranges[:, 1] - ranges[:, 0]
    J = int(lens.max()) if lens.size else 0
    jj = np.arange(J)
    valid = jj[None, :] < lens[:, None]
    tl = np.full(valid.shape, -1, np.int64)
    tl[valid] = bn.face_list.astype(np.int64)[(ranges[:, :1] + jj[None, :])[valid]]
    if face_existence is not None:
        fe = _np(face_existence, np.int32)
        keep = tl >= 0
        keep[keep] = fe[tl[keep]] != 0
        order = np.argsort(~keep, axis=1, kind="stable")                # (the kernel compacts them while staging)
        tl = np.where(np.take_along_axis(keep, order, 1), np.take_along_axis(tl, order, 1), -1)
        tl = tl[:, :int(keep.sum(1).max())]                               # (columns that hold no face anywhere)
    view = (np.arange(tl.shape[0]) // (gx * gy))[:, None]
    fs = np.where(tl >= 0, tl, 0)
    mind = np.where(tl >= 0, bn.min_depths[view * F + fs], f32(0))
    maxd = np.where(tl >= 0, bn.max_depths[view * F + fs], f32(0))
    b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    tile = ((b * gy + y // TILE) * gx + x // TILE).reshape(-1)
    return tl[tile], mind[tile].astype(f32), maxd[tile].astype(f32)


def off_plane32(rd, p0, p1, p2):
    """The hit rule's second half (dm2_hip.h, dm2_rasterize_run), float32 in the kernel's order: with E1 = p1 - p0,
    E2 = p2 - p0, n = cross(E1, E2):  dot(rd, n)^2 > (PLANE_COS2 * dot(n, n)) * dot(rd, rd)."""
    with np.errstate(invalid="ignore", over="ignore"):
        n = _cross(p1 - p0, p2 - p0)
        dn = _dot(rd, n)
        return dn * dn > (PLANE_COS2 * _dot(n, n)) * _dot(rd, rd)


def hits32(verts, faces, cand, ray_o, ray_d, rule=True):
    """-> (hit (N, J) bool, t, u, v (N, J) float32) of every candidate: ray_tri_intersection with t, u, v >= 0, u + v <= 1
    and, of those, the ones ``off_plane32`` keeps.  ``rule=False``: the hit test as it was before that rule (for counting what
    the rule removes)."""
    vs, fc = _np(verts, f32), _np(faces, np.int32)
    N, J = cand.shape
    ro, rd = _np(ray_o, f32).reshape(N, 3), _np(ray_d, f32).reshape(N, 3)
    z = np.zeros((N, J), f32)
    hit, t, u, v = np.zeros((N, J), bool), z, z.copy(), z.copy()
    step = max(1, (1 << 21) // max(J, 1))                             # (pixels per block: bounds the (block, J, 3) temporaries)
    for a in range(0, N if J else 0, step):
        c = cand[a:a + step]
        vid = fc[np.where(c >= 0, c, 0)]
        p0, p1, p2 = vs[vid[..., 0]], vs[vid[..., 1]], vs[vid[..., 2]]
        ok, t[a:a + step], u[a:a + step], v[a:a + step] = ray_tri32(ro[a:a + step, None], rd[a:a + step, None], p0, p1, p2)
        tt, uu, vv = t[a:a + step], u[a:a + step], v[a:a + step]
        with np.errstate(invalid="ignore", over="ignore"):
            h = (c >= 0) & ok & (tt >= 0) & (uu >= 0) & (vv >= 0) & (uu + vv <= f32(1))
        if rule:
            h &= off_plane32(rd[a:a + step, None], p0, p1, p2)
        hit[a:a + step] = h
    return hit, t, u, v


def _walk(hit, t, cand, mind, maxd, L):
    """The kernel's walk with its early exit: -> (N, L) column indices of the listed hits, -1 = empty."""
    N, J = hit.shape
    out = np.full((N, L), -1, np.int64)
    exhausted = np.zeros(N, bool)
    prev_t, prev_id = np.zeros(N, f32), np.full(N, -1, np.int64)
    rows = np.arange(N)
    for p in range(0, L, PASS):
        Lp = min(PASS, L - p)
        ht = np.full((N, Lp), np.inf, f32); hid = np.full((N, Lp), NO_ID, np.int64)
        hj = np.full((N, Lp), -1, np.int64); hm = np.full((N, Lp), -np.inf, f32)
        cnt = np.zeros(N, np.int64)
        bound = np.full(N, -np.inf, f32)
        done = exhausted.copy()
        j0 = 0                                                          # columns [j0, j) hold no hit: they can only stop lanes
        for j in np.nonzero(hit.any(0))[0]:
            done |= (cnt == Lp) & ((cand[:, j0:j + 1] >= 0) & (mind[:, j0:j + 1] > bound[:, None])).any(1)
            j0 = j + 1
            act = ~done & hit[:, j]
            if p > 0:
                act &= (t[:, j] > prev_t) | ((t[:, j] == prev_t) & (cand[:, j] > prev_id))
            r = np.nonzero(act)[0]
            if not len(r):
                continue
            # the hit goes in behind every held hit before it in (t, id) order (what the kernel's compare-and-swap does)
            et, eid = t[r, j], cand[r, j]
            pos = ((ht[r] < et[:, None]) | ((ht[r] == et[:, None]) & (hid[r] < eid[:, None]))).sum(1)[:, None]
            kk = np.arange(Lp)[None]
            for arr, val in ((ht, et), (hid, eid), (hj, np.full(len(r), j)), (hm, maxd[r, j])):
                a = arr[r]
                shifted = np.concatenate([a[:, :1], a[:, :-1]], 1)
                arr[r] = np.where(kk < pos, a, np.where(kk == pos, val[:, None], shifted))
            cnt[r] = np.minimum(cnt[r] + 1, Lp)
            full = r[cnt[r] == Lp]
            bound[full] = hm[full].max(1)
        out[:, p:p + Lp] = np.where(np.arange(Lp)[None] < cnt[:, None], hj, -1)
        exhausted |= cnt < Lp
        prev_t, prev_id = ht[rows, Lp - 1], hid[rows, Lp - 1]
    return out


def rasterize32(width, height, verts, faces, face_existence, verts_ndc, verts_image, ray_o, ray_d, num_layers, early_exit=False):
    """-> dict(layers (B,H,W,L) int32, cnt (B,H,W) int32, bary (B,H,W,L,3) float32, t (B,H,W,L) float32) of the contract."""
    return select(intersect(width, height, verts, faces, face_existence, verts_ndc, verts_image, ray_o, ray_d), num_layers,
                  early_exit)


def intersect(width, height, verts, faces, face_existence, verts_ndc, verts_image, ray_o, ray_d, rule=True):
    """Every pixel's candidates and their intersections (what does not depend on L)."""
    cand, mind, maxd = candidates(width, height, faces, face_existence, verts_ndc, verts_image)
    hit, t, u, v = hits32(verts, faces, cand, ray_o, ray_d, rule)
    return dict(shape=(_np(verts_ndc, f32).shape[0], int(height), int(width)), cand=cand, mind=mind, maxd=maxd, hit=hit, t=t,
                u=u, v=v)


def select(x, num_layers, early_exit=False):
    """The first L hits of ``intersect``'s candidates (rasterize32)."""
    L = int(num_layers)
    B, H, W = x["shape"]
    N = B * H * W
    cand, mind, maxd, hit, t, u, v = (x[k] for k in ("cand", "mind", "maxd", "hit", "t", "u", "v"))
    J = cand.shape[1]
    if early_exit:
        sel = _walk(hit, t, cand, mind, maxd, L)
    else:
        kt = np.where(hit, t, np.inf)
        kid = np.where(hit, cand, NO_ID)
        order = np.lexsort((kid, kt), axis=-1)[:, :L] if J else np.zeros((N, 0), np.int64)
        order = np.pad(order, ((0, 0), (0, L - order.shape[1])), constant_values=0)
        nh = np.minimum(hit.sum(1), L)
        sel = np.where(np.arange(L)[None] < nh[:, None], order, -1)
    have = sel >= 0
    s = np.where(have, sel, 0)
    take = (lambda a, fill: np.where(have, np.take_along_axis(a, s, 1), fill)) if J else (lambda a, fill: np.full(sel.shape, fill, a.dtype))
    ids = take(cand, -1).astype(np.int32)
    tt = take(t, f32(-1)).astype(f32)
    uu = take(u, f32(0)).astype(f32)
    vv = take(v, f32(0)).astype(f32)
    b0 = np.where(have, (f32(1) - uu) - vv, f32(-1)).astype(f32)
    bary = np.stack([b0, np.where(have, uu, f32(-1)), np.where(have, vv, f32(-1))], -1).astype(f32)
    return dict(layers=ids.reshape(B, H, W, L), cnt=have.sum(1).astype(np.int32).reshape(B, H, W),
                bary=bary.reshape(B, H, W, L, 3), t=tt.reshape(B, H, W, L))


def uvt64(ro, rd, p0, p1, p2):
    """Moeller-Trumbore in float64 torch (differentiable): -> (t, u, v)."""
    T, E1, E2 = ro - p0, p1 - p0, p2 - p0
    P = torch.cross(rd, E2, dim=-1)
    Q = torch.cross(T, E1, dim=-1)
    inv = 1.0 / (P * E1).sum(-1)
    return (Q * E2).sum(-1) * inv, (P * T).sum(-1) * inv, (Q * rd).sum(-1) * inv


def grads64(verts, faces, layers, ray_o, ray_d, g_bary, g_t):
    """dL/dverts (P,3) float64 of L = sum over the listed slots (0 <= f < F) of g_bary . (1 - u - v, u, v) + g_t t, the
    intersection recomputed in float64 at the float32 ray."""
    vs = torch.tensor(_np(verts, np.float64), requires_grad=True)
    fc = torch.as_tensor(_np(faces, np.int64))
    rl = _np(layers, np.int64)
    B, H, W, L = rl.shape
    F = fc.shape[0]
    m = (rl >= 0) & (rl < F)
    pix = np.nonzero(m)
    f = torch.as_tensor(rl[m])
    ro = torch.as_tensor(_np(ray_o, np.float64).reshape(B, H, W, 3)[pix[:3]])
    rd = torch.as_tensor(_np(ray_d, np.float64).reshape(B, H, W, 3)[pix[:3]])
    vid = fc[f]
    t, u, v = uvt64(ro, rd, vs[vid[:, 0]], vs[vid[:, 1]], vs[vid[:, 2]])
    gb = torch.as_tensor(_np(g_bary, np.float64)[m]) if g_bary is not None else torch.zeros((len(f), 3), dtype=torch.float64)
    gt = torch.as_tensor(_np(g_t, np.float64)[m]) if g_t is not None else torch.zeros(len(f), dtype=torch.float64)
    loss = (gb[:, 0] * (1 - u - v) + gb[:, 1] * u + gb[:, 2] * v + gt * t).sum()
    if len(f):
        loss.backward()
    return vs.grad.numpy() if vs.grad is not None else np.zeros(tuple(vs.shape), np.float64)


SCENES = ("soup", "lattice", "degenerate", "no_faces")


def scene(name):
    """The inputs the GPU tests hand the op, float32 numpy on the CPU: dict(W, H, verts, faces, fe (random existence),
    verts_ndc, verts_image, ray_o, ray_d) -- projections and rays from the oracle, so both sides read the same bits.
      soup        three cameras, views [2, 0, 2], 90x70 (not multiples of 16), lists ~30 deep (passes of 16 for L > 16)
      lattice     tet_lattice(n=4), two cameras, views [1, 0], its own existence flags
      degenerate  a soup with zero-area faces (a repeated vertex) and faces behind the camera or in front of its near plane
      no_faces    F = 0"""
    from oracle import cpu as orc
    from dmesh2_renderer_amd import scenes
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "lattice":
        W, H, views = 72, 56, [1, 0]
        ts = scenes.tet_lattice(W, H, 4, seed=scenes.SEED_BASE + 81, num_cams=2)
        verts, faces, fe = ts.verts.numpy(), ts.faces.numpy(), ts.faces_existence.numpy()
        mv, proj = ts.mv[views], ts.proj[views]
    else:
        W, H, views = (90, 70, [2, 0, 2]) if name == "soup" else (64, 40, [0])
        F = {"soup": 1000, "degenerate": 300, "no_faces": 20}[name]
        sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + 80, num_cams=max(views) + 1,
                                  depth_complexity=30.0 if name == "soup" else 4.0, shared_verts=name == "soup")
        verts, faces = sc.verts.numpy().copy(), sc.faces.numpy().copy()
        mv, proj = sc.mv[views], sc.proj[views]
        if name == "degenerate":
            faces[::7, 2] = faces[::7, 1]                                         # zero area: a repeated vertex
            behind = np.arange(3, F, 11)
            vid = faces[behind].reshape(-1)
            verts[vid, 2] = 3.5 + rng.uniform(0, 1.5, len(vid)).astype(f32)       # behind the camera (it sits at z = 3)
            near = np.arange(5, F, 13)
            verts[faces[near].reshape(-1), 2] = 2.5                               # between the camera and its near plane
        if name == "no_faces":
            faces = faces[:0]
        fe = (rng.uniform(size=faces.shape[0]) < 0.7).astype(np.int32)
    prep = orc.prepare_faces(verts, faces, mv, proj, W, H)
    ro, rd = orc.analytic_rays(mv, proj, W, H)
    return dict(W=W, H=H, verts=verts.astype(f32), faces=faces.astype(np.int32), fe=fe, verts_ndc=prep["verts_ndc"],
                verts_image=prep["verts_image"], ray_o=ro, ray_d=rd)


def near_ties(ras, rel=1e-6):
    """(B,H,W) bool: pixels whose listed hits hold two faces with |t_i - t_j| <= rel * t (rays through a shared edge or
    vertex, where the tet walk stops or may take either face)."""
    t = ras["t"]
    have = ras["layers"] >= 0
    if t.shape[-1] < 2:
        return np.zeros(t.shape[:3], bool)
    a, b = t[..., :-1].astype(np.float64), t[..., 1:].astype(np.float64)
    both = have[..., :-1] & have[..., 1:]
    return (both & (np.abs(b - a) <= rel * np.maximum(np.abs(a), np.abs(b)))).any(-1)


def prefix_violations(gen_layers, gen_cnt, ras):
    """(B,H,W) bool: pixels where generate's list is not a prefix of rasterize's."""
    gl, gc, rl = _np(gen_layers, np.int32), _np(gen_cnt, np.int32), ras["layers"]
    L = gl.shape[-1]
    n = np.minimum(gc, L)
    slot = np.arange(L)[None, None, None]
    return ((slot < n[..., None]) & (gl != rl[..., :L])).any(-1)


# ---- the tet scenes (tests/tet_scenes.py): rays through vertices, along edges and in face planes, exact ties, a camera
# inside the mesh, long tile lists ---------------------------------------------------------------------------------------------
TET_CASES = ("aligned", "holes", "inside", "flat", "duplicates", "deep", "deep_sort", "chunk_edge", "chunk_edge3")
_TET, _TET_X = {}, {}


def tet_case(name, W=None, H=None):
    """``tet_scenes.case(name)`` as ``scene()`` returns a scene -- every camera of the scene a view, projections from
    ``orc.prepare_faces``, rays from ``orc.analytic_rays``, ``fe`` the scene's own existence flags -- plus ``fe_odd`` (a seeded
    mix of 0, 1, 2, -1 and INT_MIN: any non-zero value means "exists") and the cameras ``mv``, ``proj``.  Cached: read-only."""
    key = (name, W, H)
    if key not in _TET:
        from oracle import cpu as orc
        import tet_scenes
        ts, _ = tet_scenes.case(name, W, H)
        verts, faces = ts.verts.numpy().astype(f32), ts.faces.numpy().astype(np.int32)
        mv, proj = ts.mv.numpy(), ts.proj.numpy()
        prep = orc.prepare_faces(verts, faces, mv, proj, ts.width, ts.height)
        ro, rd = orc.analytic_rays(mv, proj, ts.width, ts.height)
        fe_odd = tet_scenes.existence_tables(faces.shape[0], sum(map(ord, name)))["odd"]
        _TET[key] = dict(W=ts.width, H=ts.height, verts=verts, faces=faces, fe=ts.faces_existence.numpy().astype(np.int32),
                         fe_odd=fe_odd, verts_ndc=prep["verts_ndc"], verts_image=prep["verts_image"], ray_o=ro, ray_d=rd, mv=mv,
                         proj=proj)
    return _TET[key]


def tet_intersect(name, exist=None, rule=True, W=None, H=None):
    """``intersect`` of ``tet_case(name)`` with existence None, "fe" or "fe_odd".  Cached, as the GPU tests cache scenes."""
    key = (name, exist, rule, W, H)
    if key not in _TET_X:
        s = tet_case(name, W, H)
        _TET_X[key] = intersect(s["W"], s["H"], s["verts"], s["faces"], None if exist is None else s[exist], s["verts_ndc"],
                                s["verts_image"], s["ray_o"], s["ray_d"], rule)
    return _TET_X[key]


def tie_pairs(ras):
    """Neighbouring listed slots with exactly equal t (the face id alone orders them): -> (L - 1,) counts per slot pair
    k | k + 1."""
    t, have = ras["t"], ras["layers"] >= 0
    L = t.shape[-1]
    if L < 2:
        return np.zeros(0, np.int64)
    return (have[..., :-1] & have[..., 1:] & (t[..., :-1] == t[..., 1:])).reshape(-1, L - 1).sum(0)


def edge_hits(x):
    """Hits of ``intersect`` exactly on an edge or vertex of their face (u == 0, v == 0 or u + v == 1 in float32)
    -> (hits, pixels)."""
    u, v = x["u"], x["v"]
    with np.errstate(invalid="ignore", over="ignore"):
        e = x["hit"] & ((u == 0) | (v == 0) | (u + v == f32(1)))
    return int(e.sum()), int(e.any(1).sum())


def rule_removed(x_old, x_new):
    """What the hit rule removes: -> (hits, pixels) that ``intersect(rule=False)`` has and ``intersect()`` has not."""
    gone = x_old["hit"] & ~x_new["hit"]
    assert not (x_new["hit"] & ~x_old["hit"]).any()
    return int(gone.sum()), int(gone.any(1).sum())


def _mt64(ro, rd, p0, p1, p2):
    """Moeller-Trumbore in float64 numpy -> t, u, v, cos(ray, normal)."""
    T, E1, E2 = ro - p0, p1 - p0, p2 - p0
    P, Q = np.cross(rd, E2), np.cross(T, E1)
    n = np.cross(E1, E2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (P * E1).sum(-1)
        cos = (rd * n).sum(-1) / (np.linalg.norm(n, axis=-1) * np.linalg.norm(rd, axis=-1))
        return (Q * E2).sum(-1) * inv, (P * T).sum(-1) * inv, (Q * rd).sum(-1) * inv, cos


def unsound64(s, x):
    """Soundness of the hits of ``intersect`` result ``x`` on scene ``s`` against float64 at the float32 ray and vertices:
    -> (N, J) bool, hits with a float64 barycentric <= -1e-4 or |t - t64| > 1e-4 t + 1e-5."""
    vs, fc = s["verts"].astype(np.float64), s["faces"]
    ro, rd = s["ray_o"].astype(np.float64).reshape(-1, 3), s["ray_d"].astype(np.float64).reshape(-1, 3)
    pix, j = np.nonzero(x["hit"])
    vid = fc[x["cand"][pix, j]]
    t, u, v, _ = _mt64(ro[pix], rd[pix], vs[vid[:, 0]], vs[vid[:, 1]], vs[vid[:, 2]])
    t32 = x["t"][pix, j].astype(np.float64)
    with np.errstate(invalid="ignore"):
        good = (u > -1e-4) & (v > -1e-4) & (1.0 - u - v > -1e-4) & (np.abs(t32 - t) <= 1e-4 * t32 + 1e-5)
    bad = np.zeros(x["hit"].shape, bool)
    bad[pix[~good], j[~good]] = True
    return bad


def straddles(s):
    """(B, F) bool: faces with vertices strictly on both sides of view b's camera plane (view z = 0), in float64."""
    v = np.concatenate([s["verts"].astype(np.float64), np.ones((len(s["verts"]), 1))], 1)
    z = np.einsum("bij,pj->bpi", s["mv"].astype(np.float64), v)[..., 2]
    zf = z[:, s["faces"]]
    return (zf.max(-1) > 0) & (zf.min(-1) < 0)


def clear_hits64(s, face_existence=None, straddlers=False):
    """Float64 brute force over all faces, nothing read from the binning: the clear hits of every pixel's ray -- |cos(ray,
    normal)| > 1e-3, all three barycentrics > 1e-4, t > 1e-4, the face kept by the NDC depth cull (not max_z < -1 or
    min_z > 1 over its verts_ndc), its existence not 0, and the face not straddling the view's camera plane
    (``straddlers=True``: only the straddling ones instead).  -> (pix, face, t64) arrays, pix in (b, y, x) order.  Chunked
    within views."""
    vs, fc = s["verts"].astype(np.float64), s["faces"]
    B, H, W = s["ray_o"].shape[:3]
    ro, rd = s["ray_o"].astype(np.float64).reshape(B, H * W, 3), s["ray_d"].astype(np.float64).reshape(B, H * W, 3)
    F = fc.shape[0]
    zf = s["verts_ndc"][..., 2][:, fc]                                   # (B, F, 3)
    keep = ~((zf.max(-1) < -1) | (zf.min(-1) > 1)) & (straddles(s) == straddlers)
    if face_existence is not None:
        keep &= (np.asarray(face_existence) != 0)[None]
    out = []
    step = max(1, (1 << 21) // max(F, 1))
    for b in range(B):
        fs = np.nonzero(keep[b])[0]
        p0, p1, p2 = (vs[fc[fs, k]][None] for k in range(3))
        for a in range(0, H * W if len(fs) else 0, step):
            t, u, v, cos = _mt64(ro[b, a:a + step, None], rd[b, a:a + step, None], p0, p1, p2)
            with np.errstate(invalid="ignore"):
                m = (np.abs(cos) > 1e-3) & (u > 1e-4) & (v > 1e-4) & (1.0 - u - v > 1e-4) & (t > 1e-4)
            pi, fi = np.nonzero(m)
            out.append((b * H * W + a + pi, fs[fi], t[pi, fi]))
    if not out:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def missing64(x, clear, L=None):
    """Completeness: the clear hits (``clear_hits64``) that ``select(x, L)`` does not list although they lie nearer than a full
    list's last t -- nearer by more than 1e-4 t + 1e-5, what soundness grants a listed float32 t, so that a face at the last
    one's very distance (its duplicate, say, with the higher id) is not demanded (L None: every hit of ``x`` is listed, nothing
    is excused).  -> indices into ``clear``."""
    pix, face, t64 = clear
    N, J = x["hit"].shape
    F1 = int(max(face.max(initial=0), x["cand"].max(initial=0))) + 2
    if L is None:
        listed_key = np.nonzero(x["hit"])
        keys = listed_key[0] * F1 + x["cand"][listed_key]
        last = np.full(N, np.inf)
    else:
        r = select(x, L)
        ids = r["layers"].reshape(N, L).astype(np.int64)
        keys = (np.arange(N)[:, None] * F1 + ids)[ids >= 0]
        tl = r["t"].reshape(N, L)[:, -1].astype(np.float64)
        last = np.where(r["cnt"].reshape(N) == L, tl - (1e-4 * tl + 1e-5), np.inf)
    listed = np.isin(pix * F1 + face, keys)
    return np.nonzero(~listed & (t64 < last[pix]))[0]
