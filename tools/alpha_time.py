"""What the alpha image costs: Renderer.forward + loss.backward() at bench cfg 4 (1920 x 1080, 1 M faces, B = 1, aa_temperature 1,
K = 20, default host prep) in three variants -- no alpha; alpha in the loss; alpha returned but left out of the loss -- and
LayeredRenderer.render forward + backward at cfg 3 (1024^2, tet_lattice(n=25), L = 4 from generate) with and without alpha in
the loss.  The variants alternate step by step in one process; device events around each step, median over --reps after
--warmup.  One JSON line.

    python tools/alpha_time.py [--reps 60] [--warmup 10] [--skip-layered]
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


def renderer_steps(dev):
    W, H, F = 1920, 1080, 1_000_000
    sc = scenes.triangle_soup(W, H, F, scenes.SEED_BASE + 4).to(dev)
    r = dm2.Renderer(sc.mv, sc.proj, W, H, dev, aa_grad_buffer_size=20)
    leaves = [sc.verts.clone().requires_grad_(True), sc.verts_color.clone().requires_grad_(True),
              sc.faces_opacity.clone().requires_grad_(True), sc.faces_intense.clone().requires_grad_(True)]
    g = torch.Generator().manual_seed(1)
    wc = torch.randn((1, H, W, 3), generator=g).to(dev)
    wd = torch.randn((1, H, W), generator=g).to(dev)
    wa = torch.randn((1, H, W), generator=g).to(dev)
    pm = torch.zeros((1, 2), dtype=torch.int64, device=dev)

    def step(return_alpha, use_alpha):
        def run():
            for x in leaves:
                x.grad = None
            out = r([0], pm, W, H, leaves[0], sc.faces, leaves[1], leaves[2], leaves[3], sc.background, aa_temperature=1.0,
                    return_alpha=return_alpha)
            loss = (out[0] * wc).sum() + (out[1] * wd).sum()
            if use_alpha:
                loss = loss + (out[2] * wa).sum()
            loss.backward()
        return run
    return {"no_alpha": step(False, False), "alpha_in_loss": step(True, True), "alpha_unused": step(True, False)}


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
    wa = torch.randn((1, H, W), generator=g).to(dev)

    def step(use_alpha):
        def run():
            for x in leaves:
                x.grad = None
            out = lr.render([0], layers, ts.verts, ts.faces, *leaves, bg, return_alpha=use_alpha)
            loss = (out[0] * wc).sum() + (out[1] * wd).sum()
            if use_alpha:
                loss = loss + (out[2] * wa).sum()
            loss.backward()
        return run
    return {"layered_no_alpha": step(False), "layered_alpha_in_loss": step(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--skip-layered", action="store_true")
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"cfg4": alternate(renderer_steps(dev), opt.reps, opt.warmup)}
    c = res["cfg4"]
    res["cfg4"]["alpha_in_loss_overhead_pct"] = round(100.0 * (c["alpha_in_loss"] / c["no_alpha"] - 1.0), 2)
    res["cfg4"]["alpha_unused_overhead_pct"] = round(100.0 * (c["alpha_unused"] / c["no_alpha"] - 1.0), 2)
    if not opt.skip_layered:
        torch.cuda.empty_cache()
        lt = res["cfg3_layered"] = alternate(layered_steps(dev), opt.reps, opt.warmup)
        lt["alpha_in_loss_overhead_pct"] = round(100.0 * (lt["layered_alpha_in_loss"] / lt["layered_no_alpha"] - 1.0), 2)
    print(json.dumps(dict(tool="alpha_time", reps=opt.reps, warmup=opt.warmup, ms_fwd_bwd=res)))


if __name__ == "__main__":
    main()
