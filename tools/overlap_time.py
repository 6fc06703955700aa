"""Time Renderer.rasterize in its overlap mode next to the standard mode, and Renderer.coverage with and without the inside mask,
on the same inputs, next to Renderer.forward + backward (the path the overlap lists let the deferred path reproduce).  One JSON
line.

    python tools/overlap_time.py [--reps 20] [--warmup 3] [--skip-cfg4] [--standard-only]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags) and cfg 4 (1920x1080, 1 M-face
soup), L = 4.  Forward under no_grad; forward + backward with verts requiring grad and a random-weighted sum over bary and t (or
cov) as the loss.  The callables alternate step by step in one process; device events around each step; median and the 10th /
90th percentile over --reps after --warmup.  ``--standard-only`` times only what exists without the overlap mode (standard
rasterize, coverage without a mask, Renderer.forward), so that the same script measures a checkout from before the mode for
comparison.  Next to the times: the slots listed by either mode and the share of overlap slots off their triangle.
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


def case(r, sc, L, reps, warmup, existence=None, full_render=False, standard_only=False):
    dev = sc.verts.device
    kw = dict(faces_existence=existence)
    modes = {"standard": {}} if standard_only else {"standard": {}, "overlap": dict(overlap=True)}
    g = torch.Generator(device=dev).manual_seed(L)
    verts = sc.verts.clone().requires_grad_(True)
    fns, res = {}, dict(L=L)
    with torch.no_grad():
        ras = {m: r.rasterize([0], sc.verts, sc.faces, L, **kw, **o) for m, o in modes.items()}
    wb = torch.randn(ras["standard"][2].shape, device=dev, generator=g)
    wt = torch.randn(ras["standard"][3].shape, device=dev, generator=g)
    for m, o in modes.items():
        res[m + "_slots"] = int((ras[m][0] >= 0).sum())

        def fwd(o=o):
            with torch.no_grad():
                return r.rasterize([0], sc.verts, sc.faces, L, **kw, **o)

        def fwd_bwd(o=o):
            verts.grad = None
            out = r.rasterize([0], verts, sc.faces, L, **kw, **o)
            ((out[2] * wb).sum() + (out[3] * wt).sum()).backward()

        fns["rasterize_" + m + "_fwd"], fns["rasterize_" + m + "_fwd_bwd"] = fwd, fwd_bwd
    ids = ras["standard" if standard_only else "overlap"][0]
    inside = None if standard_only else ras["overlap"][4]
    wc = torch.randn(ids.shape, device=dev, generator=g)
    if inside is not None:
        res["off_triangle_share"] = round(int(((ids >= 0) & ~inside).sum()) / max(res["overlap_slots"], 1), 4)
    for name, ckw in (("coverage", {}),) + ((("coverage_inside", dict(inside=inside)),) if inside is not None else ()):
        def cfwd(ckw=ckw):
            with torch.no_grad():
                return r.coverage([0], ids, sc.verts, sc.faces, **ckw)

        def cfwd_bwd(ckw=ckw):
            verts.grad = None
            (r.coverage([0], ids, verts, sc.faces, **ckw) * wc).sum().backward()

        fns[name + "_fwd"], fns[name + "_fwd_bwd"] = cfwd, cfwd_bwd
    if full_render:
        pm = torch.zeros((1, 2), dtype=torch.int64, device=dev)
        gc = torch.randn((1, r.height, r.width, 3), device=dev, generator=g)

        def render_fwd():
            with torch.no_grad():
                return r([0], pm, r.width, r.height, sc.verts, sc.faces, sc.verts_color, sc.faces_opacity, sc.faces_intense[[0]],
                         sc.background, aa_temperature=1.0)

        def render_fwd_bwd():
            verts.grad = None
            color, depth = r([0], pm, r.width, r.height, verts, sc.faces, sc.verts_color, sc.faces_opacity, sc.faces_intense[[0]],
                             sc.background, aa_temperature=1.0)
            (color * gc).sum().backward()

        fns["render_fwd"], fns["render_fwd_bwd"] = render_fwd, render_fwd_bwd
    res["times"] = alternate(fns, reps, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--standard-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlap_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="overlap_time", reps=a.reps, warmup=a.warmup, standard_only=a.standard_only, device=torch.cuda.get_device_name(0))
    ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
    out["cfg3"] = case(lr, ts, 4, a.reps, a.warmup, existence=ts.faces_existence, standard_only=a.standard_only)
    del lr, ts
    torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        out["cfg4"] = case(r, sc, 4, a.reps, a.warmup, full_render=True, standard_only=a.standard_only)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
