"""Restatement of Renderer.interpolate's contract (include/dm2_hip.h: dm2_interpolate / dm2_interpolate_backward) in numpy.

A slot s = (b, y, x, l) is filled when f = render_layers[s] lies in [0, F) and the rows v_k = attr_faces[f][k] all lie in
[0, N); then out[s, c] = (bary[s,0] attr[v_0,c] + bary[s,1] attr[v_1,c]) + bary[s,2] attr[v_2,c].  Every other slot is empty:
zeros out, no gradient, its bary never used.  attr is (N, C), shared by the views, or (B, N, C), one table per view.
"""
import numpy as np

f32 = np.float32


def filled(render_layers, attr_faces, N):
    """-> (mask (B,H,W,L) of the filled slots, rows (B,H,W,L,3) int64 of attr, 0 in empty slots)."""
    rl = np.asarray(render_layers).astype(np.int64)
    af = np.asarray(attr_faces).astype(np.int64).reshape(-1, 3)
    F = af.shape[0]
    m = (rl >= 0) & (rl < F)
    rows = np.zeros(rl.shape + (3,), np.int64)
    if F:
        rows = af[np.where(m, rl, 0)]
    m = m & ((rows >= 0) & (rows < N)).all(-1)
    return m, np.where(m[..., None], rows, 0)


def _gather(attr, rows, dtype):
    """attr rows of every slot: (B,H,W,L,3,C)."""
    a = np.asarray(attr).astype(dtype)
    if a.shape[-2] == 0:
        return np.zeros(rows.shape + (a.shape[-1],), dtype)
    if a.ndim == 3:
        b = np.arange(rows.shape[0]).reshape(-1, 1, 1, 1, 1)
        return a[b, rows]
    return a[rows]


def forward(render_layers, bary, attr, attr_faces, dtype):
    """The contract's expression in ``dtype``: separate multiplies and adds, in the written order."""
    attr = np.asarray(attr)
    m, rows = filled(render_layers, attr_faces, attr.shape[-2])
    a = _gather(attr, rows, dtype)
    w = np.where(m[..., None], np.asarray(bary), 0).astype(dtype)
    p0 = (w[..., 0, None] * a[..., 0, :]).astype(dtype)
    p1 = (w[..., 1, None] * a[..., 1, :]).astype(dtype)
    p2 = (w[..., 2, None] * a[..., 2, :]).astype(dtype)
    out = ((p0 + p1).astype(dtype) + p2).astype(dtype)
    return np.where(m[..., None], out, dtype(0))


def forward32(render_layers, bary, attr, attr_faces):
    return forward(render_layers, bary, attr, attr_faces, f32)


def forward_bound(render_layers, bary, attr, attr_faces):
    """sum_k |bary_k| |attr_k| per element (float64): the scale of the three-term sum's rounding error."""
    attr = np.asarray(attr)
    m, rows = filled(render_layers, attr_faces, attr.shape[-2])
    a = np.abs(_gather(attr, rows, np.float64))
    w = np.abs(np.where(m[..., None], np.asarray(bary), 0).astype(np.float64))
    return (w[..., None] * a).sum(-2)


def grads64(render_layers, bary, attr, attr_faces, g):
    """(dL/dattr of attr's shape, dL/dbary (B,H,W,L,3)) in float64 for upstream g (B,H,W,L,C)."""
    attr = np.asarray(attr)
    N, C = attr.shape[-2], attr.shape[-1]
    m, rows = filled(render_layers, attr_faces, N)
    a = _gather(attr, rows, np.float64)
    g = np.asarray(g).astype(np.float64)
    w = np.where(m[..., None], np.asarray(bary), 0).astype(np.float64)
    dbary = np.where(m[..., None], (a * g[..., None, :]).sum(-1), 0.0)
    dattr = np.zeros(attr.shape, np.float64)
    flat = dattr.reshape(-1, C)
    contrib = w[..., None] * g[..., None, :]                                  # (B,H,W,L,3,C)
    if attr.ndim == 3:
        rows = rows + (np.arange(rows.shape[0]) * N).reshape(-1, 1, 1, 1, 1)
    sel = np.broadcast_to(m[..., None], rows.shape)
    if N:
        np.add.at(flat, rows[sel], contrib[sel])
    return dattr, dbary


def one_liner(render_layers, bary, attr, attr_faces):
    """The torch line the op replaces, on torch tensors of any dtype / device (attr (N,C) only; ids in [-1, F))."""
    ids = render_layers.long()
    img = (bary[..., None] * attr[attr_faces.long()[ids.clamp(min=0)]]).sum(-2)
    return img * (ids >= 0)[..., None].to(img.dtype)


def distinct_per_tile(render_layers, tile=16):
    """The smallest number of distinct ids over the tile x tile pixel tiles of every view."""
    rl = np.asarray(render_layers)
    B, H, W, L = rl.shape
    best = None
    for b in range(B):
        for y in range(0, H, tile):
            for x in range(0, W, tile):
                n = len(np.unique(rl[b, y:y + tile, x:x + tile]))
                best = n if best is None else min(best, n)
    return best
