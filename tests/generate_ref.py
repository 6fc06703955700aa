"""What LayeredRenderer.generate must compute, restated for the tests without the kernels' or the oracle's code.

* ``brute64`` -- float64 numpy, no tiles, no tets, no walk: every ray against every face; a ray's layers are the existing
  faces it hits, ordered by t and cut at L.  On a mesh without holes that is what the walk finds, except where a ray passes
  within rounding of an edge or a vertex: ``excusable`` marks those pixels (two hits closer along the ray than the near-tie
  margin, or a barycentric within that margin of an edge).  Margin and cap are those of
  test_gpu_rasterize.py::test_generate_is_a_prefix.
* ``walk32`` -- the tet walk (forward.cu:853-996) vectorised over pixels in float32 numpy in the kernels' operation order,
  started from given first faces / tets.  It returns the layers and, per pixel, WHY the walk ended: the tests measure their
  scenes by these causes.
* ``oracle`` / ``inputs`` -- the CPU oracle on a scene, fed what the renderer at hand computes (projection, rays).
"""
import inspect

import numpy as np
import torch

from layer_composite_ref import _cross, _dot, ray_tri32
from rasterize_ref import near_ties, prefix_violations

f32 = np.float32
MARGIN = inspect.signature(near_ties).parameters["rel"].default      # test_generate_is_a_prefix's near-tie margin
CAP = 0.001                                                           # ... and its cap on the excused share of pixels

# walk32's causes
NO_HIT, NO_TET, FULL, LEFT, CNT, BACK, NCAND0, NCAND2, CAPPED = range(9)
CAUSES = ("no first hit", "first hit without a tet to enter", "L layers found", "left through a face with no tet behind",
          "cnt != 3", "dot(ncur, rd) >= 0", "ncand == 0", "ncand >= 2", "T + 1 step cap")


def _np(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def inputs(lr, verts, bidx):
    """verts_ndc, verts_image, ray_o, ray_d (numpy) as ``lr.generate(bidx, verts, ...)`` hands them to the op (unfused prep,
    ray tensors)."""
    bidx = list(bidx)
    ndc, img = lr.compute_verts_ndc_image(verts, lr.mv[bidx], lr.proj[bidx])
    return dict(ndc=_np(ndc, f32), img=_np(img, f32), ro=_np(lr.ray_o[bidx], f32), rd=_np(lr.ray_d[bidx], f32))


def oracle(ts, inp, L, existence=None):
    """oracle.cpu.generate_render_layers_cuda(..., return_first=True) on scene ``ts`` -> dict(layers, cnt, ff, ft, bn)."""
    from oracle import cpu as orc
    ex = ts.faces_existence if existence is None else existence
    rl, rc, ff, ft, bn = orc.generate_render_layers_cuda(
        ts.width, ts.height, _np(ts.verts, f32), _np(ts.faces, np.int32), _np(ts.tets, np.int32), _np(ts.face_tets, np.int32),
        _np(ts.tet_faces, np.int32), _np(ex, np.int32), inp["ndc"], inp["img"], inp["ro"], inp["rd"], L, return_first=True)
    return dict(layers=rl, cnt=rc, ff=ff, ft=ft, bn=bn)


def list_positions(bn, ff):
    """(B,H,W) position of each pixel's first face in its tile's list (-1: no first face)."""
    B, H, W = ff.shape
    gx, gy = bn.gx, bn.gy
    pos = np.full(ff.shape, -1, np.int64)
    ranges = bn.ranges.astype(np.int64)
    for tile in range(B * gx * gy):
        b, ty, tx = tile // (gx * gy), (tile % (gx * gy)) // gx, tile % gx
        lst = bn.face_list[ranges[tile, 0]:ranges[tile, 1]].astype(np.int64)
        first = {}
        for j in range(len(lst) - 1, -1, -1):
            first[int(lst[j])] = j
        blk = ff[b, ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16]
        pos[b, ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = np.vectorize(lambda f: first.get(int(f), -1))(blk) if blk.size else blk
    return pos


def list_lengths(bn):
    r = bn.ranges.astype(np.int64)
    return r[:, 1] - r[:, 0]


# ---- float64 brute force -------------------------------------------------------------------------------------------------
def brute64(verts, faces, existence, ray_o, ray_d, L, hull=None, margin=MARGIN, chunk=512):
    """-> dict(layers (B,H,W,L) int32, cnt, t (B,H,W,L) float64, excusable (B,H,W) bool).  ``hull`` (F,) bool, the faces with
    one tet: the walk does not re-enter a mesh it has left (a jittered lattice is not convex), so a ray's layers end with
    its second hull hit, the face it leaves through."""
    v, fc = _np(verts, np.float64), _np(faces, np.int64)
    ex = _np(existence, np.int64) != 0
    ro, rd = _np(ray_o, np.float64), _np(ray_d, np.float64)
    B, H, W = ro.shape[:3]
    N, F = B * H * W, fc.shape[0]
    ro, rd = ro.reshape(N, 3), rd.reshape(N, 3)
    p0, e1, e2 = v[fc[:, 0]], v[fc[:, 1]] - v[fc[:, 0]], v[fc[:, 2]] - v[fc[:, 0]]
    layers = np.full((N, L), -1, np.int32); ts = np.full((N, L), -1.0); cnt = np.zeros(N, np.int32)
    excusable = np.zeros(N, bool)
    for s in range(0, N, chunk):
        o, d = ro[s:s + chunk, None], rd[s:s + chunk, None]                       # (M,1,3)
        with np.errstate(divide="ignore", invalid="ignore"):
            P = np.cross(d, e2[None]); T = o - p0[None]; Q = np.cross(T, e1[None])
            inv = 1.0 / (P * e1[None]).sum(-1)
            t, u, w = (Q * e2[None]).sum(-1) * inv, (P * T).sum(-1) * inv, (Q * d).sum(-1) * inv
            k = 1.0 - u - w
            ok = np.isfinite(inv)
            hit = ok & (t >= 0) & (u >= 0) & (w >= 0) & (k >= 0)
            lo = np.minimum(np.minimum(u, w), k)
            edge = ok & (t >= -margin) & (lo >= -margin) & (lo <= margin)       # on, or a hair outside, an edge
        excusable[s:s + chunk] |= edge.any(1)
        # two hits of ANY faces (the walk crosses the absent ones too) closer than the margin
        ta = np.sort(np.where(hit | edge, t, np.inf), axis=1)
        a, b = ta[:, :-1], ta[:, 1:]
        with np.errstate(invalid="ignore"):
            tie = np.isfinite(b) & (np.abs(b - a) <= margin * np.maximum(np.abs(a), np.abs(b)))
        excusable[s:s + chunk] |= tie.any(1)
        te = np.where(hit & ex[None], t, np.inf)
        if hull is not None:
            th = np.sort(np.where(hit & np.asarray(hull, bool)[None], t, np.inf), axis=1)
            te = np.where(te <= (th[:, 1:2] if th.shape[1] > 1 else np.inf), te, np.inf)
        order = np.argsort(te, axis=1, kind="stable")[:, :L]
        tt = np.take_along_axis(te, order, 1)
        have = np.isfinite(tt)
        layers[s:s + chunk, :order.shape[1]] = np.where(have, order, -1)
        ts[s:s + chunk, :order.shape[1]] = np.where(have, tt, -1.0)
        cnt[s:s + chunk] = have.sum(1)
    return dict(layers=layers.reshape(B, H, W, L), t=ts.reshape(B, H, W, L), cnt=cnt.reshape(B, H, W),
                excusable=excusable.reshape(B, H, W))


def cut(br, L):
    """brute64's result for a smaller L."""
    return dict(layers=br["layers"][..., :L], t=br["t"][..., :L], cnt=np.minimum(br["cnt"], L), excusable=br["excusable"])


def brute_violations(gen_layers, gen_cnt, br):
    """(B,H,W) bool: pixels where generate's result is not the brute force's: a listed id differs, or the count does."""
    return prefix_violations(gen_layers, gen_cnt, br) | (_np(gen_cnt, np.int32) != br["cnt"])


def check_brute(gen_layers, gen_cnt, br, what=""):
    """The gate of the brute-force comparison: every violation excusable, the excused within CAP.  -> excused share."""
    bad = brute_violations(gen_layers, gen_cnt, br)
    excused = int((bad & br["excusable"]).sum())
    print(f"{what}: {excused} of {bad.size} pixels excused ({excused / bad.size:.5%}; cap {CAP:.1%}), "
          f"{int(br['excusable'].sum())} excusable, {int((bad & ~br['excusable']).sum())} unexcused")
    assert not (bad & ~br["excusable"]).any()
    assert excused <= CAP * bad.size
    return excused / bad.size


# ---- the walk, restated with its causes ------------------------------------------------------------------------------------
def _normal32(v, faces, tets, f, t):
    """tet_face_outward_normal (auxiliary.h:382-431) on id arrays (M,) -> (M,3) float32."""
    p0, p1, p2 = v[faces[f, 0]], v[faces[f, 1]], v[faces[f, 2]]
    n = _cross(p1 - p0, p2 - p0)
    nn = np.maximum(np.sqrt(_dot(n, n)), f32(0.0001))
    n = n / nn[:, None]
    q = v[tets[t]]
    c = (((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]) * f32(0.25)
    return np.where((_dot(n, c - p0) > 0)[:, None], -n, n)


def walk32(verts, faces, tets, face_tets, tet_faces, existence, ray_o, ray_d, ff, ft, L):
    """The walk from first faces ``ff`` / first tets ``ft`` (B,H,W).  -> dict(layers (B,H,W,L), cnt, cause, last_face (the
    face the walk stood on when it ended), steps (B,H,W), visited (T,) bool)."""
    v, fc, tt = _np(verts, f32), _np(faces, np.int64), _np(tets, np.int64)
    ftt, tf, ex = _np(face_tets, np.int64), _np(tet_faces, np.int64), _np(existence, np.int64) != 0
    shape = ff.shape
    N, T = ff.size, tt.shape[0]
    ro, rd = _np(ray_o, f32).reshape(N, 3), _np(ray_d, f32).reshape(N, 3)
    cf, ct = _np(ff, np.int64).reshape(N).copy(), _np(ft, np.int64).reshape(N).copy()
    cause = np.full(N, -1, np.int64)
    cause[cf < 0] = NO_HIT
    cause[(cf >= 0) & (ct < 0)] = NO_TET
    active = cause < 0
    layers = np.full((N, max(L, 1)), -1, np.int32)
    ndone, steps = np.zeros(N, np.int64), np.zeros(N, np.int64)
    visited = np.zeros(T, bool)
    step = 0

    def end(idx, why):
        cause[idx] = why
        active[idx] = False

    with np.errstate(all="ignore"):
        while active.any():
            step += 1
            idx = np.nonzero(active)[0]
            if step > T + 1:
                end(idx, CAPPED)
                break
            steps[idx] += 1
            e = ex[cf[idx]]
            w = idx[e & (ndone[idx] < L)]
            layers[w, ndone[w]] = cf[w]
            ndone[idx] += e
            full = e & (ndone[idx] >= L)
            end(idx[full], FULL)
            left = ~full & (ct[idx] < 0)
            end(idx[left], LEFT)
            idx = idx[~full & ~left]
            if not len(idx):
                continue
            f, t = cf[idx], ct[idx]
            visited[t] = True
            faces4 = tf[t]                                                    # (M,4)
            same = faces4 == f[:, None]
            bad = (~same).sum(1) != 3
            back = _dot(_normal32(v, fc, tt, f, t), rd[idx]) >= 0
            ncand = np.zeros(len(idx), np.int64)
            nxt = np.full(len(idx), -1, np.int64)
            for i in range(4):
                of = faces4[:, i]
                ok, th, u, vv = ray_tri32(ro[idx], rd[idx], v[fc[of, 0]], v[fc[of, 1]], v[fc[of, 2]])
                hit = ok & (th >= 0) & (u >= 0) & (vv >= 0) & (u + vv <= f32(1))
                c = ~same[:, i] & hit & (_dot(_normal32(v, fc, tt, of, t), rd[idx]) > 0)
                ncand += c
                nxt = np.where(c, of, nxt)
            end(idx[bad], CNT)
            end(idx[~bad & back], BACK)
            go = ~bad & ~back
            end(idx[go & (ncand == 0)], NCAND0)
            end(idx[go & (ncand >= 2)], NCAND2)
            go &= ncand == 1
            g = idx[go]
            pair = ftt[nxt[go]]
            cf[g] = nxt[go]
            ct[g] = np.where(pair[:, 0] != t[go], pair[:, 0], np.where(pair[:, 1] != t[go], pair[:, 1], -1))
    return dict(layers=layers[:, :L].reshape(shape + (L,)), cnt=ndone.astype(np.int32).reshape(shape), cause=cause.reshape(shape),
                last_face=cf.reshape(shape), steps=steps.reshape(shape), visited=visited)


def walk_scene(ts, inp, orc_out, L, existence=None):
    ex = ts.faces_existence if existence is None else existence
    return walk32(ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ex, inp["ro"], inp["rd"], orc_out["ff"], orc_out["ft"], L)
