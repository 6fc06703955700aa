"""Restatement of Renderer.rasterize's contract (include/dm2_hip.h: dm2_rasterize_run) for the tests.

* ``candidates`` -- each pixel's tile list from the oracle's own binning (``oracle.cpu.Binning(..., key_min_depth=True)``:
  the plan's bbox bins and depth cull, lists in min-depth order), with the faces of existence 0 taken out.
* ``rasterize32`` -- float32 Moeller-Trumbore in the device's operation order (``layer_composite_ref.ray_tri32``; numpy float32
  is IEEE and uncontracted like the kernels built with -ffp-contract=off), the hit test, the (t, face id) order, the first L
  hits.  ``early_exit=True`` walks each pixel's list the way the kernel does instead -- passes of 16, each stopping at the
  first face whose min depth lies beyond the largest max depth of a full set of held hits -- so that a test can show the stop
  changes nothing; the contract is the result without it.
* ``grads64`` -- float64 torch autograd of (bary, t) w.r.t. verts over given (pixel, face) pairs.
"""
import numpy as np
import torch

from layer_composite_ref import ray_tri32

f32 = np.float32
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
    view = (np.arange(tl.shape[0]) // (gx * gy))[:, None]
    fs = np.where(tl >= 0, tl, 0)
    mind = np.where(tl >= 0, bn.min_depths[view * F + fs], f32(0))
    maxd = np.where(tl >= 0, bn.max_depths[view * F + fs], f32(0))
    b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    tile = ((b * gy + y // TILE) * gx + x // TILE).reshape(-1)
    return tl[tile], mind[tile].astype(f32), maxd[tile].astype(f32)


def hits32(verts, faces, cand, ray_o, ray_d):
    """-> (hit (N, J) bool, t, u, v (N, J) float32) of every candidate: ray_tri_intersection with t, u, v >= 0, u + v <= 1."""
    vs, fc = _np(verts, f32), _np(faces, np.int32)
    N, J = cand.shape
    ro, rd = _np(ray_o, f32).reshape(N, 3), _np(ray_d, f32).reshape(N, 3)
    if J == 0:
        z = np.zeros((N, 0), f32)
        return np.zeros((N, 0), bool), z, z, z
    vid = fc[np.where(cand >= 0, cand, 0)]
    ok, t, u, v = ray_tri32(ro[:, None], rd[:, None], vs[vid[..., 0]], vs[vid[..., 1]], vs[vid[..., 2]])
    with np.errstate(invalid="ignore", over="ignore"):
        hit = (cand >= 0) & ok & (t >= 0) & (u >= 0) & (v >= 0) & (u + v <= f32(1))
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
        for j in range(J):
            done |= (cand[:, j] >= 0) & (cnt == Lp) & (mind[:, j] > bound)
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


def intersect(width, height, verts, faces, face_existence, verts_ndc, verts_image, ray_o, ray_d):
    """Every pixel's candidates and their intersections (what does not depend on L)."""
    cand, mind, maxd = candidates(width, height, faces, face_existence, verts_ndc, verts_image)
    hit, t, u, v = hits32(verts, faces, cand, ray_o, ray_d)
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
