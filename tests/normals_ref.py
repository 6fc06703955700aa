"""Restatement of Renderer.vertex_adjacency / Renderer.vertex_normals (include/dm2_hip.h: dm2_vertex_normals) in numpy.

  adjacency(faces, P)    the inverted index by a plain Python loop
  normals32(...)         the forward in float32, every multiply and add rounded separately, in the contract's order: the
                         kernels must give these bits
  normals64(...)         the same sums in float64, with the sums of absolute values a rounding bound needs
  grads64(...)           dL/dverts in float64 from the contract's formulas, with the abs-evaluated sum of its terms
  loss64(...)            sum(g * normals) in float64 as a plain function of verts (for central differences)
and the meshes the tests share: octahedron(), fan(valence), edge_mesh().

Contract: a face is valid when its three ids lie in [0, P); N = (p1 - p0) x (p2 - p0) with components e1.y * e2.z - e1.z * e2.y,
...; s_p = ((0 + N_c0) + N_c1) + ... over the vertex's corners in ``corners`` order; len = sqrt((s.x s.x + s.y s.y) + s.z s.z);
normalize: s / len where len > 0 and finite, zeros elsewhere; otherwise s.  Gradient: d_p = (g_p - n_p (n_p . g_p)) / len (or g_p),
D = (d_v0 + d_v1) + d_v2 per valid face, c1 = e2 x D, c2 = D x e1, c0 = -(c1 + c2), dL/dverts[p] = the sum of its corners' c_k."""
import numpy as np

f32 = np.float32


def adjacency(faces, P):
    """(offsets (P+1,), corners (3F,)) int32: corner numbers 3 f + k by (vertex id, corner number) ascending, invalid faces' last."""
    faces = np.asarray(faces).reshape(-1, 3)
    lists = [[] for _ in range(P + 1)]
    for f, row in enumerate(faces):
        ok = all(0 <= int(v) < P for v in row)
        for k, v in enumerate(row):
            lists[int(v) if ok else P].append(3 * f + k)
    offsets = np.zeros(P + 1, np.int32)
    for p in range(P):
        offsets[p + 1] = offsets[p] + len(lists[p])
    corners = np.array([c for lst in lists for c in lst], dtype=np.int32).reshape(-1)
    return offsets, corners


def _valid(faces, P):
    return ((faces >= 0) & (faces < P)).all(1) if len(faces) else np.zeros(0, bool)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _abscross(a, b):
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)


def _edges(verts, faces, dtype):
    """(valid, e1, e2) of every face (zeros for invalid ones), in ``dtype``."""
    v = np.asarray(verts, dtype).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ok = _valid(faces, v.shape[0])
    fc = np.where(ok[:, None], faces, 0)
    zero = np.zeros((len(faces), 3), dtype)
    if v.shape[0] == 0:
        return ok, zero, zero.copy(), fc
    p0, p1, p2 = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
    return ok, np.where(ok[:, None], p1 - p0, zero), np.where(ok[:, None], p2 - p0, zero), fc


def normals32(verts, faces, offsets, corners, normalize=True):
    """The forward, float32, bit for bit (one pass per list position: every vertex adds its j-th corner's N)."""
    P = np.asarray(verts).reshape(-1, 3).shape[0]
    ok, e1, e2, _ = _edges(verts, faces, f32)
    with np.errstate(all="ignore"):
        N = _cross(e1, e2).astype(f32)
        N[~ok] = 0
        s = np.zeros((P, 3), f32)
        beg = np.asarray(offsets[:-1], np.int64)
        cnt = np.asarray(offsets[1:], np.int64) - beg
        for j in range(int(cnt.max()) if P else 0):
            m = cnt > j
            s[m] = s[m] + N[np.asarray(corners)[beg[m] + j] // 3]
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]).astype(f32)
        if not normalize:
            return s
        good = (ln > 0) & np.isfinite(ln)
        return np.where(good[:, None], s / np.where(good, ln, f32(1))[:, None], f32(0)).astype(f32)


def _sums64(verts, faces):
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    P = v.shape[0]
    ok, e1, e2, fc = _edges(verts, faces, np.float64)
    N, Na = _cross(e1, e2), _abscross(e1, e2)
    s, sa = np.zeros((P, 3)), np.zeros((P, 3))
    for k in range(3):
        np.add.at(s, fc[ok, k], N[ok])
        np.add.at(sa, fc[ok, k], Na[ok])
    return ok, e1, e2, fc, s, sa


def normals64(verts, faces, normalize=True):
    """(normals, s, s_abs) in float64: s the sum of the face normals, s_abs the sum of their abs-evaluated components."""
    ok, e1, e2, fc, s, sa = _sums64(verts, faces)
    ln = np.sqrt((s * s).sum(1))
    good = (ln > 0) & np.isfinite(ln)
    n = np.where(good[:, None], s / np.where(good, ln, 1.0)[:, None], 0.0)
    return (n if normalize else s), s, sa


def grads64(verts, faces, g, normalize=True):
    """(dL/dverts, sabs) in float64: the contract's formulas, and the same formulas evaluated on absolute values (every
    subtraction an addition), with n and len taken as exact: sum|terms| of the criterion, nothing added for the forward's own
    rounding of n (the backward has to evaluate n and len well enough for that, which is why it does so in double)."""
    g = np.asarray(g, np.float64).reshape(-1, 3)
    ok, e1, e2, fc, s, sa = _sums64(verts, faces)
    P = s.shape[0]
    if normalize:
        ln = np.sqrt((s * s).sum(1))
        good = (ln > 0) & np.isfinite(ln)
        l1 = np.where(good, ln, 1.0)[:, None]
        n = np.where(good[:, None], s / l1, 0.0)
        d = np.where(good[:, None], (g - n * (n * g).sum(1, keepdims=True)) / l1, 0.0)
        da = (np.abs(g) + np.abs(n) * (np.abs(n) * np.abs(g)).sum(1, keepdims=True)) / l1
        da = np.where(good[:, None], da, 0.0)
    else:
        d, da = g, np.abs(g)
    grad, sabs = np.zeros((P, 3)), np.zeros((P, 3))
    if P == 0 or not ok.any():
        return grad, sabs
    D = d[fc[:, 0]] + d[fc[:, 1]] + d[fc[:, 2]]
    Da = da[fc[:, 0]] + da[fc[:, 1]] + da[fc[:, 2]]
    c1, c2 = _cross(e2, D), _cross(D, e1)
    a1, a2 = _abscross(e2, Da), _abscross(Da, e1)
    for k, (c, a) in enumerate(((-(c1 + c2), a1 + a2), (c1, a1), (c2, a2))):
        np.add.at(grad, fc[ok, k], c[ok])
        np.add.at(sabs, fc[ok, k], a[ok])
    return grad, sabs


def loss64(verts, faces, g, normalize=True):
    return float((np.asarray(g, np.float64) * normals64(verts, faces, normalize)[0]).sum())


def central_differences(verts, faces, g, normalize=True, h=1e-6):
    v = np.asarray(verts, np.float64).copy()
    out = np.zeros_like(v)
    for idx in np.ndindex(*v.shape):
        keep = v[idx]
        v[idx] = keep + h
        hi = loss64(v, faces, g, normalize)
        v[idx] = keep - h
        lo = loss64(v, faces, g, normalize)
        v[idx] = keep
        out[idx] = (hi - lo) / (2 * h)
    return out


# ---- meshes -----------------------------------------------------------------------------------------------------------------------
def octahedron():
    """Vertices +-e_i, eight faces oriented outwards: every sum is made of integers, the normals are the six axis directions."""
    verts = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    faces = []
    for sx, ix in ((1, 0), (-1, 1)):
        for sy, iy in ((1, 2), (-1, 3)):
            for sz, iz in ((1, 4), (-1, 5)):
                faces.append([ix, iy, iz] if sx * sy * sz > 0 else [ix, iz, iy])
    return verts, np.array(faces, np.int32)


def fan(valence, seed=0):
    """A cone of ``valence`` triangles round vertex 0 (its list is ``valence`` long, every rim vertex's two), slightly jittered."""
    rng = np.random.default_rng(seed)
    a = np.arange(valence) * (2 * np.pi / valence)
    rim = np.stack([np.cos(a), np.sin(a), np.zeros(valence)], 1) + rng.uniform(-0.02, 0.02, (valence, 3))
    verts = np.concatenate([[[0.0, 0.0, 0.7]], rim]).astype(f32)
    k = np.arange(valence)
    faces = np.stack([np.zeros(valence, np.int64), 1 + k, 1 + (k + 1) % valence], 1).astype(np.int32)
    return verts, faces


def edge_mesh(seed=3):
    """Every special case in one mesh of P = 14 vertices: two isolated vertices (12, 13), a zero-area face (collinear corners), a
    face with a repeated id, faces with an id out of range (negative and >= P), and vertex 8, whose only two faces are the same
    triangle with opposite orientations: its sum cancels exactly (zeros out, and its own upstream gradient goes nowhere)."""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-1, 1, (14, 3)).astype(f32)
    verts[3], verts[4], verts[5] = (0.25, 0.5, -0.5), (0.5, 0.25, 0.0), (0.75, 0.0, 0.5)     # collinear: e2 = 2 e1, N = 0 exactly
    faces = np.array([[0, 1, 2], [2, 1, 3], [0, 2, 6], [6, 2, 7], [3, 4, 5],        # the last: zero area
                      [1, 1, 4], [7, 6, 6],                                          # repeated ids
                      [0, 14, 1], [-1, 2, 3], [5, 6, 99],                            # out of range
                      [8, 9, 10], [8, 10, 9],                                        # vertex 8: exact cancellation
                      [9, 10, 11], [10, 9, 0], [4, 7, 11], [5, 0, 7]], np.int32)
    return verts, faces
