"""Time LayeredRenderer's layer compositor (dm2_layers_composite + backward) against the plain torch gather-and-composite
of the same contract with autograd (what a user of the layered path writes without the op).  One JSON line.

    python tools/layer_composite_time.py [--size 1024] [--n 25] [--layers 4] [--reps 50] [--warmup 10]

Default: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), L = 4 from generate, B = 1).  Device events around each call,
median over --reps after --warmup; the torch path is checked against the op (pixels off by > 1e-5 counted, at most 0.1 %)
before it is timed.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import dmesh2_renderer_amd as dm2  # noqa: E402
from dmesh2_renderer_amd import _C, scenes  # noqa: E402


def torch_composite(layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background, ray_o, ray_d):
    """The contract in torch ops: gather per-layer face tables, Moeller-Trumbore, clamp code 0, front-to-back blend."""
    B, H, W, L = layers.shape
    F = faces.shape[0]
    valid = (layers >= 0) & (layers < F)
    fs = torch.where(valid, layers, torch.zeros_like(layers)).long()
    vid = faces.long()[fs]                                                   # (B,H,W,L,3)
    p0, p1, p2 = verts[vid[..., 0]], verts[vid[..., 1]], verts[vid[..., 2]]
    ro, rd = ray_o[..., None, :], ray_d[..., None, :]
    T_, E1, E2 = ro - p0, p1 - p0, p2 - p0
    P = torch.cross(rd.expand_as(E2), E2, dim=-1)
    Q = torch.cross(T_, E1, dim=-1)
    den = (P * E1).sum(-1)
    ok = den != 0
    inv = 1.0 / torch.where(ok, den, torch.ones_like(den))
    u = (P * T_).sum(-1) * inv
    v = (Q * rd).sum(-1) * inv
    hit = valid & ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    w0 = 1 - u - v
    col = (w0[..., None] * verts_color[vid[..., 0]] + u[..., None] * verts_color[vid[..., 1]] + v[..., None] * verts_color[vid[..., 2]])
    bidx = torch.arange(B, device=layers.device).view(B, 1, 1, 1)
    iC = col * faces_intense[bidx, fs][..., None]
    z = verts_ndc[..., 2]
    iD = w0 * z[bidx, vid[..., 0]] + u * z[bidx, vid[..., 1]] + v * z[bidx, vid[..., 2]]
    alpha = torch.where(hit, faces_opacity[fs], torch.zeros((), device=layers.device))
    T = torch.ones((B, H, W), device=layers.device)
    C = torch.zeros((B, H, W, 3), device=layers.device)
    D = torch.zeros((B, H, W), device=layers.device)
    for l in range(L):
        a = torch.where(T < 1e-4, torch.zeros_like(alpha[..., l]), alpha[..., l])       # the T_EPS stop
        C = C + iC[..., l, :] * (a * T)[..., None]
        D = D + iD[..., l] * a * T
        T = T * (1 - a)
    return C + T[..., None] * background, D + T


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--n", type=int, default=25)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("layer_composite_time.py needs a GPU")
    dev = "cuda"
    W = H = a.size
    ts = scenes.tet_lattice(W, H, a.n, seed=scenes.SEED_BASE + 3).to(dev)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, dev)
    layers, _ = lr.generate([0], ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, a.layers)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    g = torch.Generator().manual_seed(0)
    vc = torch.rand((P, 3), generator=g).to(dev)
    op = torch.rand((F,), generator=g).to(dev)
    it = (0.5 + torch.rand((1, F), generator=g)).to(dev)
    bg = torch.tensor([0.1, 0.3, 0.7], device=dev)
    ndc, _ = lr.compute_verts_ndc_image(ts.verts, ts.mv[[0]], ts.proj[[0]])
    ndc = ndc.contiguous()
    ro, rd = lr.ray_o[[0]].contiguous(), lr.ray_d[[0]].contiguous()
    gc, gd = torch.randn((1, H, W, 3), generator=g).to(dev), torch.randn((1, H, W), generator=g).to(dev)

    def hip_fwd():
        return _C.composite_layers_cuda(layers, ts.verts, ts.faces, vc, op, it, ndc, bg, ro, rd)

    def hip_fwd_bwd():
        c, d, _, nc = hip_fwd()
        return _C.composite_layers_backward_cuda(layers, ts.verts, ts.faces, vc, op, it, ndc, bg, ro, rd, nc, gc, gd)

    leaves = [t.clone().requires_grad_(True) for t in (vc, op, it, ndc)]

    def torch_fwd():
        with torch.no_grad():
            return torch_composite(layers, ts.verts, ts.faces, vc, op, it, ndc, bg, ro, rd)

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        c, d = torch_composite(layers, ts.verts, ts.faces, *leaves, bg, ro, rd)
        torch.autograd.backward([c, d], [gc, gd])

    c_hip, d_hip = hip_fwd()[:2]
    c_t, d_t = torch_fwd()
    # (torch's own operation order may flip the hit decision of a ray that grazes an edge: count, do not demand bits)
    off = ((c_hip - c_t).abs().amax(-1) > 1e-5) | ((d_hip - d_t).abs() > 1e-5)
    mismatch = int(off.sum())
    if mismatch > 1e-3 * off.numel():
        raise SystemExit(f"torch restatement disagrees with the op at {mismatch} pixels")
    N, L = H * W, a.layers
    slots = int(((layers >= 0) & (layers < F)).sum())
    # bytes the op requests, counted from the shapes: per pixel its ids, ray and outputs; per valid (pixel, layer) slot the
    # gathered face rows (neighbouring pixels share faces, so most of these are served from cache, not HBM)
    fwd_bytes = N * (L * 4 + 24 + 24) + slots * (12 + 36 + 36 + 12 + 8)       # ids, rays, outputs (colour, depth, T, n); per slot
    bwd_bytes = N * (L * 4 + 24 + 16 + 4) + slots * (12 + 36 + 36 + 12 + 8)   # ids, rays, upstream grads, n_contrib; per slot
    out = dict(cfg=3 if (a.size, a.n, a.layers) == (1024, 25, 4) else None, W=W, H=H, n=a.n, L=L, B=1, P=P, F=F,
               layer_slots=slots, pixels_covered=int((hip_fwd()[3] > 0).sum()),
               hip_fwd_ms=round(timed(hip_fwd, a.reps, a.warmup), 4), hip_fwd_bwd_ms=round(timed(hip_fwd_bwd, a.reps, a.warmup), 4),
               torch_fwd_ms=round(timed(torch_fwd, a.reps, a.warmup), 4),
               torch_fwd_bwd_ms=round(timed(torch_fwd_bwd, a.reps, a.warmup), 4),
               fwd_bytes_model=fwd_bytes, bwd_bytes_model=bwd_bytes, reps=a.reps, warmup=a.warmup,
               torch_vs_hip_pixels_off=mismatch, device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
