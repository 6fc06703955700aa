#!/usr/bin/env python3
"""What the camera-matrix gradients cost (dm2_prepare_faces_backward_camera), as one JSON line:

  prep_backward_ms     the fused prep's backward alone at cfg 4's P, B = 1 and B = 8: verts only (today's call), verts +
                       camera, camera only (upstream: verts_ndc and verts_image gradients, as the default path sends them)
  step_ms              Renderer.forward + loss.backward() at cfg 4 with mv / proj requiring grad and without, alternating in
                       one process (median of the per-round times)

  python tools/camera_grad_time.py [--rounds 7] [--iters 10]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import dmesh2_renderer_amd as dm2  # noqa: E402
from dmesh2_renderer_amd import _C, scenes  # noqa: E402


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, H, F, ci = bench.CONFIGS["cfg4"]
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + ci).to(dev)
    P = sc.verts.shape[0]
    faces = sc.faces.to(torch.int32)
    out = {"config": "cfg4", "P": P, "F": F, "prep_backward_ms": {}, "step_ms": {}}

    for B in (1, 8):
        mv, proj = sc.mv[[0] * B].contiguous(), sc.proj[[0] * B].contiguous()
        g_ndc, g_img = torch.randn((B, P, 3), device=dev), torch.randn((B, P, 2), device=dev)
        kw = dict(g_verts_ndc=g_ndc, g_verts_image=g_img)
        runs = {
            "verts": lambda: _C.prepare_faces_backward(sc.verts, faces, mv, proj, W, H, **kw),
            "verts_camera": lambda: _C.prepare_faces_backward(sc.verts, faces, mv, proj, W, H, need_camera=True, **kw),
            "camera_only": lambda: _C.prepare_faces_backward(sc.verts, faces, mv, proj, W, H, need_verts=False, need_camera=True, **kw),
        }
        res = {k: [] for k in runs}
        for _ in range(opt.rounds):
            for k, fn in runs.items():
                res[k].append(timed(fn, opt.iters * 5))
        out["prep_backward_ms"][f"B{B}"] = {k: round(median(v), 4) for k, v in res.items()}

    g = torch.Generator().manual_seed(scenes.SEED_BASE + 100 + ci)
    wc, wd = torch.randn((1, H, W, 3), generator=g).to(dev), torch.randn((1, H, W), generator=g).to(dev)
    pm = torch.zeros((1, 2), dtype=torch.int64, device=dev)
    steps = {}
    for name, cam_grad in (("camera_grad", True), ("no_camera_grad", False)):
        mv, proj = sc.mv.clone().requires_grad_(cam_grad), sc.proj.clone().requires_grad_(cam_grad)
        r = dm2.Renderer(mv, proj, W, H, dev)
        leaves = [t.clone().requires_grad_(True) for t in (sc.verts, sc.verts_color, sc.faces_opacity, sc.faces_intense)]

        def one(r=r, leaves=leaves, mv=mv, proj=proj):
            for t in leaves + [mv, proj]:
                t.grad = None
            color, depth = r([0], pm, W, H, leaves[0], sc.faces, leaves[1], leaves[2], leaves[3], sc.background,
                             aa_temperature=bench.AA_TEMPERATURE)
            ((color * wc).sum() + (depth * wd).sum()).backward()
        steps[name] = one
    res = {k: [] for k in steps}
    for _ in range(opt.rounds):
        for k, fn in steps.items():
            res[k].append(timed(fn, opt.iters))
    out["step_ms"] = {k: round(median(v), 4) for k, v in res.items()}
    out["step_ms"]["camera_grad_overhead_pct"] = round(100.0 * (out["step_ms"]["camera_grad"] / out["step_ms"]["no_camera_grad"] - 1.0), 3)
    out["step_ms_rounds"] = {k: [round(x, 4) for x in v] for k, v in res.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
