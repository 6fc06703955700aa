"""Time Renderer.rasterize (dm2_rasterize_run + dm2_rasterize_backward): forward under no_grad and forward + backward (a
loss on bary and t), next to LayeredRenderer.generate on the same scene.  One JSON line.

    python tools/rasterize_time.py [--reps 30] [--warmup 5] [--skip-cfg4]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4; generate next to it)
and cfg 4 (1920x1080, 1 M-face soup, L = 4 and L = 16).  Device events around each call (host prep included), median over
--reps after --warmup.
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
    return round(statistics.median(ms), 4)


def rasterize_case(r, verts, faces, L, fe, reps, warmup):
    v = verts.clone().requires_grad_(True)
    g = torch.Generator(device="cuda").manual_seed(L)
    with torch.no_grad():
        ids, cnt, bary, t = r.rasterize([0], v, faces, L, faces_existence=fe)
    gb = torch.randn(bary.shape, device="cuda", generator=g)
    gt = torch.randn(t.shape, device="cuda", generator=g)

    def fwd():
        with torch.no_grad():
            return r.rasterize([0], v, faces, L, faces_existence=fe)

    def fwd_bwd():
        v.grad = None
        _, _, b, tt = r.rasterize([0], v, faces, L, faces_existence=fe)
        torch.autograd.backward([b, tt], [gb, gt])

    return dict(L=L, listed=int(cnt.sum()), pixels_full=int((cnt == L).sum()), fwd_ms=timed(fwd, reps, warmup),
                fwd_bwd_ms=timed(fwd_bwd, reps, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-cfg4", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rasterize_time.py needs a GPU")
    dev = "cuda"
    out = dict(reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
    c3 = rasterize_case(lr, ts.verts, ts.faces, 4, ts.faces_existence, a.reps, a.warmup)
    gen = lambda: lr.generate([0], ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, ts.faces_existence, 4)
    gl, gc = gen()
    c3.update(F=int(ts.faces.shape[0]), generate_ms=timed(gen, a.reps, a.warmup), generate_listed=int(gc.sum()))
    out["cfg3"] = c3
    del lr, ts
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        out["cfg4"] = [rasterize_case(r, sc.verts, sc.faces, L, None, a.reps, a.warmup) for L in (4, 16)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
