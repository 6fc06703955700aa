"""What the per-face blend weights cost (Renderer.forward(..., return_face_weights=True)).

Renderer.forward alone under torch.no_grad() and Renderer.forward + loss.backward(), with and without the weights, at bench
cfg 4 (1920 x 1080, 1 M faces, B = 1, aa_temperature 1, K = 20, default host prep), cfg 2 (512 x 512, 50 k faces) and a
256 x 256 / 2 k-face soup (triangles of ~130 pixels: the forward's class-by-class route); LayeredRenderer.render forward
(no_grad) and forward + backward at cfg 3 (1024^2, tet_lattice(n=25), L = 4 from generate).  The variants of one scene
without and with weights alternate step by step in one process (forward-only and forward + backward steps are timed in
separate runs: they size the binning buffer differently); device events around each step, median over --reps after
--warmup.  One JSON line.

    python tools/face_weights_time.py [--reps 60] [--warmup 10] [--scenes cfg4,cfg2,soup256_2k,cfg3_layered]
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
from dmesh2_renderer_amd import scenes  # noqa: E402


def alternate(fns, reps, warmup):
    """{name: median ms} of the callables in ``fns``, run round-robin (one step of each per round)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def renderer_steps(dev, W, H, F, seed):
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + seed).to(dev)
    r = dm2.Renderer(sc.mv, sc.proj, W, H, dev, aa_grad_buffer_size=20)
    leaves = [sc.verts.clone().requires_grad_(True), sc.verts_color.clone().requires_grad_(True),
              sc.faces_opacity.clone().requires_grad_(True), sc.faces_intense.clone().requires_grad_(True)]
    g = torch.Generator().manual_seed(1)
    wc = torch.randn((1, H, W, 3), generator=g).to(dev)
    wd = torch.randn((1, H, W), generator=g).to(dev)
    pm = torch.zeros((1, 2), dtype=torch.int64, device=dev)

    def fwd(weights):
        def run():
            with torch.no_grad():
                r([0], pm, W, H, sc.verts, sc.faces, sc.verts_color, sc.faces_opacity, sc.faces_intense, sc.background,
                  aa_temperature=1.0, return_face_weights=weights)
        return run

    def fwd_bwd(weights):
        def run():
            for x in leaves:
                x.grad = None
            out = r([0], pm, W, H, leaves[0], sc.faces, leaves[1], leaves[2], leaves[3], sc.background, aa_temperature=1.0,
                    return_face_weights=weights)
            ((out[0] * wc).sum() + (out[1] * wd).sum()).backward()
        return run
    return [{"fwd": fwd(False), "fwd_weights": fwd(True)}, {"fwd_bwd": fwd_bwd(False), "fwd_bwd_weights": fwd_bwd(True)}]


def layered_steps(dev):
    W = H = 1024
    ts = scenes.tet_lattice(W, H, 25, seed=scenes.SEED_BASE + 3, num_cams=1).to(dev)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, W, H, dev)
    layers, _ = lr.generate([0], ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, 4)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    g = torch.Generator().manual_seed(2)
    leaves = [torch.rand((P, 3), generator=g).to(dev).requires_grad_(True),
              (0.05 + 0.9 * torch.rand((F,), generator=g)).to(dev).requires_grad_(True),
              (0.5 + torch.rand((1, F), generator=g)).to(dev).requires_grad_(True)]
    bg = torch.tensor([0.1, 0.3, 0.7], device=dev)
    wc = torch.randn((1, H, W, 3), generator=g).to(dev)
    wd = torch.randn((1, H, W), generator=g).to(dev)

    def fwd(weights):
        def run():
            with torch.no_grad():
                lr.render([0], layers, ts.verts, ts.faces, *leaves, bg, return_face_weights=weights)
        return run

    def fwd_bwd(weights):
        def run():
            for x in leaves:
                x.grad = None
            out = lr.render([0], layers, ts.verts, ts.faces, *leaves, bg, return_face_weights=weights)
            ((out[0] * wc).sum() + (out[1] * wd).sum()).backward()
        return run
    return [{"fwd": fwd(False), "fwd_weights": fwd(True)}, {"fwd_bwd": fwd_bwd(False), "fwd_bwd_weights": fwd_bwd(True)}]


def timed(groups, reps, warmup):
    t = {}
    for g in groups:
        t.update(alternate(g, reps, warmup))
    return overheads(t)


def overheads(t):
    t["fwd_overhead_pct"] = round(100.0 * (t["fwd_weights"] / t["fwd"] - 1.0), 2)
    t["fwd_bwd_overhead_pct"] = round(100.0 * (t["fwd_bwd_weights"] / t["fwd_bwd"] - 1.0), 2)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scenes", default="cfg4,cfg2,soup256_2k,cfg3_layered")
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    soups = {"cfg4": (1920, 1080, 1_000_000, 4), "cfg2": (512, 512, 50_000, 2), "soup256_2k": (256, 256, 2_000, 5)}
    res = {}
    for name in opt.scenes.split(","):
        if name == "cfg3_layered":
            res[name] = timed(layered_steps(dev), opt.reps, opt.warmup)
        else:
            res[name] = timed(renderer_steps(dev, *soups[name]), opt.reps, opt.warmup)
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool="face_weights_time", reps=opt.reps, warmup=opt.warmup, ms=res)))


if __name__ == "__main__":
    main()
