"""Restatement of the layer-compositing contract (include/dm2_hip.h: dm2_layers_composite) for the tests.

Two parts:
* ``forward32`` -- float32, vectorised numpy, in the device's operation order (numpy float32 arithmetic is IEEE and
  uncontracted, like the kernels built with -ffp-contract=off): Moeller-Trumbore, the clamp's code 0, the blend and the
  T_EPS stop.  It decides which (pixel, layer) pairs blend and gives the forward values the kernel must match bit for bit.
* ``grads64`` -- float64 torch autograd over those decisions: the reference gradients w.r.t. verts_color, faces_opacity,
  faces_intense and verts_ndc (z).  The barycentrics are the float32 pass's (constants: no gradient reaches verts).
"""
import numpy as np
import torch

T_EPS = np.float32(0.0001)
f32 = np.float32


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def ray_tri32(ro, rd, p0, p1, p2):
    """ray_tri_intersection (dm2_device_math.h) on float32 arrays (..., 3) -> ok, t, u, v."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        T = ro - p0; E1 = p1 - p0; E2 = p2 - p0
        P = _cross(rd, E2); Q = _cross(T, E1)
        denom = _dot(P, E1)
        ok = denom != f32(0)
        inv = f32(1) / np.where(ok, denom, f32(1))
        t = _dot(Q, E2) * inv
        u = _dot(P, T) * inv
        v = _dot(Q, rd) * inv
    return ok, t.astype(f32), u.astype(f32), v.astype(f32)


def clamp_code32(u, v):
    """clamp_bary_uv's region code (dm2_device_math.h), vectorised; the first match wins."""
    with np.errstate(invalid="ignore", over="ignore"):
        conds = [
            (u >= 0) & (v >= 0) & (u + v <= f32(1)),
            (u <= 0) & (v <= 0),
            ((u >= 1) & (v <= 0)) | ((v >= 0) & (v <= u - f32(1))),
            ((u <= 0) & (v >= 1)) | ((u >= 0) & (v >= u + f32(1))),
            (u <= 0) & (v <= 1) & (v >= 0),
            (u <= 1) & (u >= 0) & (v <= 0),
        ]
    return np.select(conds, [0, 1, 2, 3, 4, 5], default=6).astype(np.int32)


def _np(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def forward32(render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background, ray_o, ray_d):
    """-> dict(color (B,H,W,3), depth_raw, final_T, n_contrib, blend (B,H,W,L) bool, u, v (B,H,W,L) float32)."""
    rl = _np(render_layers, np.int32)
    B, H, W, L = rl.shape
    vs, fc, vc = _np(verts, f32), _np(faces, np.int32), _np(verts_color, f32)
    op, it, ndc, bg = _np(faces_opacity, f32), _np(faces_intense, f32), _np(verts_ndc, f32), _np(background, f32)
    ro, rd = _np(ray_o, f32).reshape(B, H, W, 3), _np(ray_d, f32).reshape(B, H, W, 3)
    F = fc.shape[0]
    valid = (rl >= 0) & (rl < F)
    fs = np.where(valid, rl, 0)
    bidx = np.arange(B).reshape(B, 1, 1, 1)
    if F > 0:
        vid = fc[fs]                                                        # (B,H,W,L,3)
        p = [vs[vid[..., i]] for i in range(3)]
        ok, _, u, v = ray_tri32(ro[..., None, :], rd[..., None, :], p[0], p[1], p[2])
        code = clamp_code32(u, v)
        hit = valid & ok & (code == 0)
        i0 = (f32(1) - u) - v
        w = (i0, u, v)
        col = [vc[vid[..., i]] for i in range(3)]                           # (B,H,W,L,3) each
        bc = ((w[0][..., None] * col[0] + w[1][..., None] * col[1]) + w[2][..., None] * col[2]).astype(f32)
        inten = it[bidx, fs]
        iC = (bc * inten[..., None]).astype(f32)
        z = [ndc[bidx, vid[..., i], 2] for i in range(3)]
        iD = ((w[0] * z[0] + w[1] * z[1]) + w[2] * z[2]).astype(f32)
        alpha = op[fs]
    else:
        hit = np.zeros(rl.shape, bool)
        u = v = iD = alpha = np.zeros(rl.shape, f32)
        iC = np.zeros(rl.shape + (3,), f32)
    T = np.ones((B, H, W), f32)
    C = np.zeros((B, H, W, 3), f32)
    D = np.zeros((B, H, W), f32)
    done = np.zeros((B, H, W), bool)
    nc = np.zeros((B, H, W), np.int32)
    blend = np.zeros(rl.shape, bool)
    for l in range(L):
        act = hit[..., l] & ~done
        a, Tm = alpha[..., l], T
        C = np.where(act[..., None], C + (iC[..., l, :] * a[..., None]) * Tm[..., None], C).astype(f32)
        D = np.where(act, D + (iD[..., l] * a) * Tm, D).astype(f32)
        T = np.where(act, Tm * (f32(1) - a), Tm).astype(f32)
        nc = np.where(act, l + 1, nc)
        done = done | (act & (T < T_EPS))
        blend[..., l] = act
    color = (C + T[..., None] * bg).astype(f32)
    depth = (D + T * f32(1)).astype(f32)
    return dict(color=color, depth_raw=depth, final_T=T, n_contrib=nc.astype(np.int32), blend=blend, u=u, v=v, fs=fs)


def composite64(fwd, faces, verts_color, faces_opacity, faces_intense, verts_ndc_z, background):
    """float64 torch restatement over the float32 pass's decisions -> (color, depth_raw); differentiable w.r.t. verts_color
    (P,3), faces_opacity (F), faces_intense (B,F) and verts_ndc_z (B,P)."""
    blend = torch.from_numpy(fwd["blend"])
    B, H, W, L = blend.shape
    fs = torch.from_numpy(fwd["fs"].astype(np.int64))
    u = torch.from_numpy(np.where(fwd["blend"], fwd["u"], 0).astype(np.float64))     # (no inf / NaN off the blended pairs)
    v = torch.from_numpy(np.where(fwd["blend"], fwd["v"], 0).astype(np.float64))
    fc = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    bg = torch.as_tensor(np.asarray(background), dtype=torch.float64)
    T = torch.ones((B, H, W), dtype=torch.float64)
    C = torch.zeros((B, H, W, 3), dtype=torch.float64)
    D = torch.zeros((B, H, W), dtype=torch.float64)
    bidx = torch.arange(B).view(B, 1, 1)
    for l in range(L):
        act = blend[..., l]
        if not bool(act.any()):
            continue
        f = fs[..., l]
        vid = fc[f] if fc.shape[0] else torch.zeros(f.shape + (3,), dtype=torch.long)
        w = (1 - u[..., l] - v[..., l], u[..., l], v[..., l])
        bc = sum(w[i][..., None] * verts_color[vid[..., i]] for i in range(3))
        iC = bc * faces_intense[bidx, f][..., None]
        iD = sum(w[i] * verts_ndc_z[bidx, vid[..., i]] for i in range(3))
        a = torch.where(act, faces_opacity[f], torch.zeros((), dtype=torch.float64))
        C = C + iC * (a * T)[..., None]
        D = D + iD * a * T
        T = T * (1 - a)
    return C + T[..., None] * bg, D + T


def grads64(fwd, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background, g_color, g_depth):
    """Reference gradients: dict(verts_color (P,3), faces_opacity (F), faces_intense (B,F), verts_ndc (B,P,3) [z only])."""
    leaves = dict(verts_color=torch.tensor(_np(verts_color, np.float64), requires_grad=True),
                  faces_opacity=torch.tensor(_np(faces_opacity, np.float64), requires_grad=True),
                  faces_intense=torch.tensor(_np(faces_intense, np.float64), requires_grad=True),
                  verts_ndc_z=torch.tensor(_np(verts_ndc, np.float64)[..., 2].copy(), requires_grad=True))
    color, depth = composite64(fwd, _np(faces, np.int64), leaves["verts_color"], leaves["faces_opacity"], leaves["faces_intense"],
                               leaves["verts_ndc_z"], _np(background, np.float64))
    loss = (color * torch.from_numpy(_np(g_color, np.float64))).sum() + (depth * torch.from_numpy(_np(g_depth, np.float64))).sum()
    loss.backward()
    out = {k: leaves[k].grad.numpy() for k in ("verts_color", "faces_opacity", "faces_intense")}
    gz = leaves["verts_ndc_z"].grad.numpy()
    out["verts_ndc"] = np.zeros(gz.shape + (3,), np.float64)
    out["verts_ndc"][..., 2] = gz
    return out


def ortho_scene(B=2, H=6, W=7, L=5, F=9, seed=0, holes=True, crowded=False):
    """Orthographic rays (origin (x, y, 0), direction -z) over [0,1]^2 and F triangles at distinct depths covering parts of
    it; layers: hand-built lists with holes, out-of-range and repeated ids.  ``crowded``: every triangle's xy scaled by 5
    about its centroid (circumradius 3), so that (nearly) every face covers the whole unit square and every listed id blends:
    with F in the hundreds or thousands a 16 x 16 tile then blends about F (1 - exp(-256 L / F)) distinct faces."""
    rng = np.random.RandomState(seed)
    ys, xs = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    ro = np.zeros((B, H, W, 3), np.float32); ro[..., 0] = xs; ro[..., 1] = ys
    rd = np.zeros((B, H, W, 3), np.float32); rd[..., 2] = -1
    P = 3 * F
    verts = np.zeros((P, 3), np.float32)
    for f in range(F):
        c = rng.uniform(0.2, 0.8, 2)
        for k in range(3):
            ang = 2 * np.pi * k / 3 + rng.uniform(0, 1)
            verts[3 * f + k, :2] = c + 0.6 * np.array([np.cos(ang), np.sin(ang)])
        verts[3 * f:3 * f + 3, 2] = -1.0 - 0.1 * f + rng.uniform(-0.02, 0.02, 3)
    if crowded:
        tri = verts.reshape(F, 3, 3)                                            # (a view: the faces are vertex triples in order)
        c = tri[:, :, :2].mean(1, keepdims=True)
        tri[:, :, :2] = (c + 5 * (tri[:, :, :2] - c)).astype(np.float32)
    faces = np.arange(P, dtype=np.int32).reshape(F, 3)
    layers = rng.randint(0, F, (B, H, W, L)).astype(np.int32)
    if holes:
        m = rng.uniform(size=layers.shape)
        layers[m < 0.15] = -1
        layers[(m >= 0.15) & (m < 0.22)] = F + 3
        layers[(m >= 0.22) & (m < 0.27)] = -7
    inputs = dict(render_layers=layers, verts=verts, faces=faces,
                  verts_color=rng.uniform(0, 1, (P, 3)).astype(np.float32),
                  faces_opacity=rng.uniform(0.1, 0.9, F).astype(np.float32),
                  faces_intense=rng.uniform(0.5, 1.5, (B, F)).astype(np.float32),
                  verts_ndc=rng.uniform(-1, 1, (B, P, 3)).astype(np.float32),
                  background=np.array([0.2, 0.5, 0.9], np.float32), ray_o=ro, ray_d=rd)
    return inputs


TILE = 16                   # the layer kernels' tile: one block, one face table


def distinct_blended_per_tile(fwd):
    """-> (smallest, largest) number of distinct blended faces (``fwd["blend"]``, ``fwd["fs"]``) over the 16 x 16 tiles of
    every view: what a block of the layer kernels asks of its face table (dm2_face_table.h)."""
    blend, fs = fwd["blend"], fwd["fs"]
    B, H, W, _ = blend.shape
    counts = []
    for b in range(B):
        for y in range(0, H, TILE):
            for x in range(0, W, TILE):
                m = blend[b, y:y + TILE, x:x + TILE]
                counts.append(len(np.unique(fs[b, y:y + TILE, x:x + TILE][m])))
    return min(counts), max(counts)


# The crowded cases of the GPU tests (B = 2, 48 x 64: twelve tiles a view).  "overflow": every tile blends more distinct faces
# than the table has slots; "nearly_full": fewer than it has slots but more than 0.8 of them, so that probe chains fail for
# some faces while free slots remain and both scatter routes mix inside a tile.  opacity: uniform range of faces_opacity
# (L = 12: small, so that lists do not end at T_EPS after a few layers).
CROWDED = {
    "overflow_L4": dict(F=4000, L=4, kind="overflow"),
    "overflow_L12": dict(F=4000, L=12, kind="overflow", opacity=(0.02, 0.3)),
    "nearly_full_L4": dict(F=600, L=4, kind="nearly_full"),
}


def crowded_case(name):
    """-> (inputs of forward32, kind) of a CROWDED case: the crowded ortho_scene with, as in the hand-built lists of the GPU
    tests, a face repeated within a pixel's list (every fifth row: slot 1 = slot 0) and opacities of exactly 1 and 0 (every
    97th face each)."""
    c = CROWDED[name]
    F = c["F"]
    sc = ortho_scene(B=2, H=48, W=64, L=c["L"], F=F, seed=0, holes=False, crowded=True)
    if "opacity" in c:
        sc["faces_opacity"] = np.random.RandomState(1).uniform(*c["opacity"], F).astype(np.float32)
    sc["faces_opacity"][0::97] = 1.0
    sc["faces_opacity"][50::97] = 0.0
    rl = sc["render_layers"]
    rl[:, ::5, :, 1] = rl[:, ::5, :, 0]
    return sc, c["kind"]


def check_crowded(kind, lo, hi, slots):
    """The condition a crowded case relies on, on the restatement's counts alone."""
    if kind == "overflow":
        assert lo > slots, (lo, hi, slots)
    else:
        assert hi <= slots and lo > 0.8 * slots, (lo, hi, slots)
