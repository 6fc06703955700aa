"""Restatement of Renderer.bary_derivatives' contract (include/dm2_hip.h: dm2_bary_derivatives_window) in numpy.

render_layers (B,H,W,L) int32, verts (P,3), faces (F,3), cam (B,32) = inv(mv) (16, row-major) then inv(proj) (16) per view, the
frame (full_W, full_H), patch_min (B,2) or None -> dbary_dx, dbary_dy (B,H,W,L,3): the derivatives of (1 - u - v, u, v) with
respect to the pixel's x and y.  The unnormalised ray direction D = w - ro is affine in the pixel position; with T = ro - p0,
E1 = p1 - p0, E2 = p2 - p0, a = E2 x T, b = T x E1, c = E2 x E1:

    u = D.a / D.c     v = D.b / D.c     du/dX = (g.a - u (g.c)) / D.c     dv/dX = (g.b - v (g.c)) / D.c,   g = dD/dX

``forward`` follows the header's operation order to the letter in ``dtype`` (float32: the contract itself; float64: the same
formula from the same float32 camera block and vertices).  ``uv64`` is float64 Moeller-Trumbore on the normalised ray of a
fractional pixel position, written from the rasterizer's form (P = rd x E2, Q = T x E1), for central differences.
"""
import numpy as np

f32 = np.float32


def camera_block(mv, proj):
    """(B,32) float32: inv(mv) then inv(proj) of each view, inverted in float64 and rounded once."""
    imv = np.linalg.inv(np.asarray(mv, np.float64)).reshape(-1, 16)
    ipr = np.linalg.inv(np.asarray(proj, np.float64)).reshape(-1, 16)
    return np.ascontiguousarray(np.concatenate([imv, ipr], 1).astype(f32))


def scene_cameras(name):
    """(mv, proj) (B,4,4) of the views of rasterize_ref.scene(name) ("soup", "lattice"), as that function selects them."""
    from dmesh2_renderer_amd import scenes
    if name == "lattice":
        ts = scenes.tet_lattice(72, 56, 4, seed=scenes.SEED_BASE + 81, num_cams=2)
        views = [1, 0]
        return ts.mv[views].numpy(), ts.proj[views].numpy()
    assert name == "soup", name
    views = [2, 0, 2]
    sc = scenes.triangle_soup(90, 70, 1000, scenes.SEED_BASE + 80, num_cams=3, depth_complexity=30.0, shared_verts=True)
    return sc.mv[views].numpy(), sc.proj[views].numpy()


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _gather(render_layers, verts, faces, dtype):
    """-> (live (B,H,W,L) bool, p0, p1, p2: lists of three (B,H,W,L) arrays of ``dtype``; vertex 0 in empty slots)."""
    rl = np.asarray(render_layers).astype(np.int64)
    verts, faces = np.asarray(verts), np.asarray(faces).astype(np.int64)
    P, F = verts.shape[0], faces.shape[0]
    live = (rl >= 0) & (rl < F)
    if F == 0 or P == 0:
        z = [np.zeros(rl.shape, dtype)] * 3
        return np.zeros(rl.shape, bool), z, z, z
    vid = faces[np.where(live, rl, 0)]
    live = live & ((vid >= 0) & (vid < P)).all(-1)
    vid = np.where(live[..., None], vid, 0)
    vs = verts.astype(dtype)
    return (live,) + tuple([vs[vid[..., k], i] for i in range(3)] for k in range(3))


def _rays(cam, B, H, W, full_W, full_H, patch_min, dtype, X=None, Y=None):
    """D = w - ro (unnormalised), ro, gX, gY as lists of three arrays broadcastable to (B,H,W,1), in the header's order.  X, Y:
    frame positions (B,H,W) to use instead of the integer pixels' (fractional ones for central differences)."""
    f = dtype
    cam = np.asarray(cam).astype(f)
    pm = np.zeros((B, 2), np.int64) if patch_min is None else np.asarray(patch_min).astype(np.int64)
    if X is None:
        X = np.broadcast_to((np.arange(W)[None, None, :] + pm[:, 0][:, None, None]).astype(f), (B, H, W))
        Y = np.broadcast_to((np.arange(H)[None, :, None] + pm[:, 1][:, None, None]).astype(f), (B, H, W))
    X, Y = np.asarray(X, f)[..., None], np.asarray(Y, f)[..., None]
    e = lambda k: cam[:, k].reshape(B, 1, 1, 1)
    imv = [e(k) for k in range(16)]
    ipr = [e(16 + k) for k in range(16)]
    Wf, Hf = f(full_W), f(full_H)
    h = [((X + f(0.5)) / Wf * f(2.0)) - f(1.0), ((Y + f(0.5)) / Hf * f(2.0)) - f(1.0), f(-1.0), f(1.0)]
    v = [((h[0] * ipr[4 * j] + h[1] * ipr[4 * j + 1]) + h[2] * ipr[4 * j + 2]) + h[3] * ipr[4 * j + 3] for j in range(4)]
    w = [((v[0] * imv[4 * k] + v[1] * imv[4 * k + 1]) + v[2] * imv[4 * k + 2]) + v[3] * imv[4 * k + 3] for k in range(3)]
    ro = [imv[3], imv[7], imv[11]]
    D = _sub(w, ro)
    sx, sy = f(2.0) / Wf, f(2.0) / Hf
    gX = [sx * (((imv[4 * k] * ipr[0] + imv[4 * k + 1] * ipr[4]) + imv[4 * k + 2] * ipr[8]) + imv[4 * k + 3] * ipr[12]) for k in range(3)]
    gY = [sy * (((imv[4 * k] * ipr[1] + imv[4 * k + 1] * ipr[5]) + imv[4 * k + 2] * ipr[9]) + imv[4 * k + 3] * ipr[13]) for k in range(3)]
    return D, ro, gX, gY


def forward(render_layers, verts, faces, cam, full_W, full_H, patch_min=None, dtype=f32, parts=False):
    """The contract in ``dtype`` -> (dbary_dx, dbary_dy) (B,H,W,L,3); ``parts``: also dict(live, u, v, Dc, gcx, gcy)."""
    rl = np.asarray(render_layers)
    B, H, W, L = rl.shape
    live, p0, p1, p2 = _gather(rl, verts, faces, dtype)
    D, ro, gX, gY = _rays(cam, B, H, W, full_W, full_H, patch_min, dtype)
    with np.errstate(all="ignore"):
        T, E1, E2 = _sub(ro, p0), _sub(p1, p0), _sub(p2, p0)
        a, b, c = _cross(E2, T), _cross(T, E1), _cross(E2, E1)
        Dc = _dot(D, c)
        ok = live & (Dc != 0)
        r = dtype(1.0) / Dc
        u, v = _dot(D, a) * r, _dot(D, b) * r
        out = []
        gcs = []
        for g in (gX, gY):
            gc = _dot(g, c)
            du = (_dot(g, a) - u * gc) * r
            dv = (_dot(g, b) - v * gc) * r
            d0 = -(du + dv)
            out.append(np.where(ok[..., None], np.stack([d0, du, dv], -1), dtype(0)).astype(dtype))
            gcs.append(np.broadcast_to(gc, ok.shape))
    if parts:
        return out[0], out[1], dict(live=ok, u=np.where(ok, u, 0), v=np.where(ok, v, 0), Dc=np.where(ok, Dc, 1), gcx=gcs[0], gcy=gcs[1])
    return out[0], out[1]


def forward32(render_layers, verts, faces, cam, full_W, full_H, patch_min=None):
    return forward(render_layers, verts, faces, cam, full_W, full_H, patch_min, f32)


def forward64(render_layers, verts, faces, cam, full_W, full_H, patch_min=None, parts=False):
    return forward(render_layers, verts, faces, cam, full_W, full_H, patch_min, np.float64, parts)


def uv64(render_layers, verts, faces, cam, full_W, full_H, X, Y):
    """(u, v, eu, ev) (B,H,W,L) float64 of each listed slot by Moeller-Trumbore in the rasterizer's form, on analytic_ray's
    normalised ray (length + 1e-6) of the frame position (X, Y) (B,H,W) float64 -- any real position; eu, ev: a bound on the
    float64 rounding error of u and v."""
    rl = np.asarray(render_layers)
    B, H, W, L = rl.shape
    live, p0, p1, p2 = _gather(rl, verts, faces, np.float64)
    D, ro, _, _ = _rays(cam, B, H, W, full_W, full_H, None, np.float64, X, Y)
    ln = np.sqrt(_dot(D, D)) + 1e-6
    rd = [d / ln for d in D]
    with np.errstate(all="ignore"):
        T, E1, E2 = _sub(ro, p0), _sub(p1, p0), _sub(p2, p0)
        Pv, Q = _cross(rd, E2), _cross(T, E1)
        den = _dot(Pv, E1)
        inv = 1.0 / den
        u, v = _dot(Pv, T) * inv, _dot(Q, rd) * inv
        # what float64 rounding can do to u and v: every product of the numerators is at most |rd| |E2| |T| (|T| |E1| |rd|), of the
        # denominator |rd| |E2| |E1|, in magnitude; 16 roundings of eps64 each cover the cross products, the sums and the division
        n = lambda a: np.sqrt(_dot(a, a))
        nrd, nT, nE1, nE2 = n(rd), n(T), n(E1), n(E2)
        k = 16 * 2.0 ** -53 / np.abs(den)
        eu = k * (nrd * nE2 * nT + np.abs(u) * nrd * nE2 * nE1)
        ev = k * (nT * nE1 * nrd + np.abs(v) * nrd * nE2 * nE1)
    z = lambda a: np.where(live, a, 0.0)
    return z(u), z(v), z(eu), z(ev)
