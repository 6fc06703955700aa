"""Time render windows on the deferred path next to the full-frame call plus crop.  One JSON line.

    python tools/window_time.py [--reps 30] [--warmup 5]

Scene: SURVEY.md 8(d) cfg 4 (1920x1080, 1 M-face soup).  Windows of 256 x 256 and 128 x 128 at the unaligned origin (837, 411).
Per window: Renderer.rasterize (L = 4) forward under no_grad and forward + backward (a loss on bary and t) with ``patch_min``,
next to the same through the full-frame call and a crop of its four outputs; Renderer.coverage forward and forward + backward
on the window's ids with ``patch_min``, next to the full-frame call on the full frame's ids and a crop.  The callables run
round-robin (one step of each per round); device events around each call (host prep included); median, p10 and p90 over --reps
after --warmup.
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

ORIGIN = (837, 411)
SIZES = (256, 128)
L = 4


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


def case(r, sc, size, reps, warmup):
    dev = sc.verts.device
    x0, y0 = ORIGIN
    pm = torch.tensor([[x0, y0]], dtype=torch.int32, device=dev)
    kw = dict(patch_min=pm, patch_width=size, patch_height=size)
    crop = lambda a: a[:, y0:y0 + size, x0:x0 + size].contiguous()
    verts = sc.verts.clone().requires_grad_(True)
    with torch.no_grad():
        ids_w, cnt_w, bary_w, t_w = r.rasterize([0], sc.verts, sc.faces, L, **kw)
        ids_f = r.rasterize([0], sc.verts, sc.faces, L)[0]
    g = torch.Generator(device=dev).manual_seed(size)
    gb = torch.randn(bary_w.shape, device=dev, generator=g)
    gt = torch.randn(t_w.shape, device=dev, generator=g)
    gc = torch.randn(ids_w.shape, device=dev, generator=g)

    def ras_window_fwd():
        with torch.no_grad():
            return r.rasterize([0], sc.verts, sc.faces, L, **kw)

    def ras_full_crop_fwd():
        with torch.no_grad():
            return [crop(a) for a in r.rasterize([0], sc.verts, sc.faces, L)]

    def ras_window_fwd_bwd():
        verts.grad = None
        _, _, b, tt = r.rasterize([0], verts, sc.faces, L, **kw)
        torch.autograd.backward([b, tt], [gb, gt])

    def ras_full_crop_fwd_bwd():
        verts.grad = None
        _, _, b, tt = r.rasterize([0], verts, sc.faces, L)
        torch.autograd.backward([crop(b), crop(tt)], [gb, gt])

    def cov_window_fwd():
        with torch.no_grad():
            return r.coverage([0], ids_w, sc.verts, sc.faces, patch_min=pm)

    def cov_full_crop_fwd():
        with torch.no_grad():
            return crop(r.coverage([0], ids_f, sc.verts, sc.faces))

    def cov_window_fwd_bwd():
        verts.grad = None
        (r.coverage([0], ids_w, verts, sc.faces, patch_min=pm) * gc).sum().backward()

    def cov_full_crop_fwd_bwd():
        verts.grad = None
        (crop(r.coverage([0], ids_f, verts, sc.faces)) * gc).sum().backward()

    fns = dict(rasterize_window_fwd=ras_window_fwd, rasterize_full_crop_fwd=ras_full_crop_fwd,
               rasterize_window_fwd_bwd=ras_window_fwd_bwd, rasterize_full_crop_fwd_bwd=ras_full_crop_fwd_bwd,
               coverage_window_fwd=cov_window_fwd, coverage_full_crop_fwd=cov_full_crop_fwd,
               coverage_window_fwd_bwd=cov_window_fwd_bwd, coverage_full_crop_fwd_bwd=cov_full_crop_fwd_bwd)
    same = bool((ids_w == crop(ids_f)).all())
    return dict(size=size, origin=list(ORIGIN), L=L, listed=int(cnt_w.sum()), ids_equal_crop=same, times=alternate(fns, reps, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_time.py needs a GPU")
    dev = "cuda"
    sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
    r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
    out = dict(tool="window_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0), scene="cfg4",
               F=int(sc.faces.shape[0]), cases=[case(r, sc, s, a.reps, a.warmup) for s in SIZES])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
