"""Time Renderer.coverage (dm2_coverage + dm2_coverage_backward, with the projection in front and its backward behind, as the
module runs them) on rasterize's output, next to two yardsticks on the same inputs: Renderer.rasterize (the stage that made the
lists) and, at cfg 4, Renderer.forward + backward (the path that evaluates the same areas, on more pairs).  One JSON line.

    python tools/coverage_time.py [--reps 20] [--warmup 3] [--skip-cfg4]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4) and cfg 4 (1920x1080,
1 M-face soup, L = 4 and L = 16).  Forward under no_grad; forward + backward with verts requiring grad and a random-weighted sum
over cov as the loss.  The callables alternate step by step in one process; device events around each step; median and the 10th /
90th percentile over --reps after --warmup.  Next to the times: the share of partially covered slots (the only ones the backward
clips with a Jacobian), and a byte model -- ids in and cov out per slot, three faces entries and three float2 of verts_image per
distinct listed (view, face) -- with the rate it makes at the forward's median (the projection's bytes are not in the model).
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
    """{name: {ms, p10, p90}} of the callables in ``fns``, run round-robin (one step of each per round)."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k in ms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fns[k]()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    out = {}
    for k, v in ms.items():
        v = sorted(v)
        out[k] = dict(ms=round(statistics.median(v), 4), p10=round(v[len(v) // 10], 4), p90=round(v[(9 * len(v)) // 10], 4))
    return out


def case(r, sc, L, reps, warmup, existence=None, full_render=False):
    dev = sc.verts.device
    with torch.no_grad():
        ids = r.rasterize([0], sc.verts, sc.faces, L, faces_existence=existence)[0]
        cov = r.coverage([0], ids, sc.verts, sc.faces)
    g = torch.Generator(device=dev).manual_seed(L)
    w = torch.randn(cov.shape, device=dev, generator=g)
    verts = sc.verts.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            return r.coverage([0], ids, sc.verts, sc.faces)

    def fwd_bwd():
        verts.grad = None
        (r.coverage([0], ids, verts, sc.faces) * w).sum().backward()

    def rasterize():
        with torch.no_grad():
            return r.rasterize([0], sc.verts, sc.faces, L, faces_existence=existence)

    fns = dict(coverage_fwd=fwd, coverage_fwd_bwd=fwd_bwd, rasterize=rasterize)
    if full_render:
        pm = torch.zeros((1, 2), dtype=torch.int64, device=dev)
        gc = torch.randn((1, r.height, r.width, 3), device=dev, generator=g)

        def render_fwd_bwd():
            verts.grad = None
            color, depth = r([0], pm, r.width, r.height, verts, sc.faces, sc.verts_color, sc.faces_opacity, sc.faces_intense[[0]],
                             sc.background, aa_temperature=1.0)
            (color * gc).sum().backward()

        fns["render_fwd_bwd"] = render_fwd_bwd
    filled = ids >= 0
    slots, nfilled = ids.numel(), int(filled.sum())
    partial = int(((cov > 0) & (cov < 1)).sum())
    distinct = int(torch.unique(ids[filled]).numel())
    model = 8 * slots + 36 * distinct
    res = dict(L=L, slots=slots, filled=nfilled, partial_share=round(partial / max(nfilled, 1), 4), distinct_faces=distinct,
               bytes_fwd=model, times=alternate(fns, reps, warmup))
    res["fwd_GBps"] = round(model / (res["times"]["coverage_fwd"]["ms"] * 1e-3) / 1e9, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg4", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coverage_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="coverage_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
    out["cfg3"] = [case(lr, ts, 4, a.reps, a.warmup, existence=ts.faces_existence)]
    del lr, ts
    torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        out["cfg4"] = [case(r, sc, 4, a.reps, a.warmup, full_render=True), case(r, sc, 16, a.reps, a.warmup)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
