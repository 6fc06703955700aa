"""Time Renderer.interpolate (dm2_interpolate + dm2_interpolate_backward) next to the torch line it replaces,

    (bary[..., None] * attr[faces[ids.clamp(min=0)].long()]).sum(-2)

on rasterize's output: forward under no_grad and forward + backward (attr and bary both requiring grad), attr shared by the
views, C = 3 and C = 16.  One JSON line.

    python tools/interpolate_time.py [--reps 20] [--warmup 3] [--skip-cfg4]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4) and cfg 4 (1920x1080,
1 M-face soup, L = 4).  The op and the torch line alternate step by step in one process on the same inputs; device events
around each step; median and the 10th / 90th percentile over --reps after --warmup.  Where the torch line runs out of
memory the point says so instead of a time.  Next to the times: the bytes a call requests (ids, bary, attr_faces rows,
gathered attr rows, out) and the global atomics the attr backward issues (one per (tile, face) pair, vertex and channel)
against slots x 3 x C.
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
    """{name: {ms, p10, p90} or {error}} of the callables in ``fns``, run round-robin (one step of each per round)."""
    failed = {}
    for k, fn in fns.items():
        try:
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
        except torch.cuda.OutOfMemoryError:
            failed[k] = dict(error="out of memory")
            torch.cuda.empty_cache()
    ms = {k: [] for k in fns if k not in failed}
    for _ in range(reps):
        for k in ms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fns[k]()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    out = dict(failed)
    for k, v in ms.items():
        v = sorted(v)
        out[k] = dict(ms=round(statistics.median(v), 4), p10=round(v[len(v) // 10], 4), p90=round(v[(9 * len(v)) // 10], 4))
    return out


def torch_line(ids, bary, attr, faces):
    return (bary[..., None] * attr[faces[ids.clamp(min=0)].long()]).sum(-2)


def tile_face_pairs(ids, F):
    """distinct (16 x 16 tile, face) pairs over the filled slots: the attr backward flushes 3 x C atomics for each."""
    B, H, W, L = ids.shape
    ys = torch.arange(H, device=ids.device).view(1, H, 1, 1) // 16
    xs = torch.arange(W, device=ids.device).view(1, 1, W, 1) // 16
    bs = torch.arange(B, device=ids.device).view(B, 1, 1, 1)
    tile = (bs * ((H + 15) // 16) + ys) * ((W + 15) // 16) + xs
    key = (tile * F + ids.long())[ids >= 0]
    return int(torch.unique(key).numel())


def case(r, ids, bary, faces, P, C, reps, warmup):
    dev = ids.device
    g = torch.Generator(device=dev).manual_seed(C)
    attr = torch.randn((P, C), device=dev, generator=g).requires_grad_(True)
    b = bary.clone().requires_grad_(True)
    gout = torch.randn(tuple(ids.shape) + (C,), device=dev, generator=g)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(ids, b, attr, faces)
        return run

    def fwd_bwd(fn):
        def run():
            attr.grad = None
            b.grad = None
            fn(ids, b, attr, faces).backward(gout)
        return run

    op = lambda i, w, a, f: r.interpolate(i, w, a, f)
    slots, filled = ids.numel(), int((ids >= 0).sum())
    pairs = tile_face_pairs(ids, faces.shape[0])
    res = dict(C=C, slots=slots, filled=filled,
               fwd=alternate(dict(op=fwd(op), torch=fwd(torch_line)), reps, warmup),
               fwd_bwd=alternate(dict(op=fwd_bwd(op), torch=fwd_bwd(torch_line)), reps, warmup),
               requested_bytes_fwd=dict(ids=4 * slots, bary=12 * slots, attr_faces_rows=12 * filled, attr_rows=12 * C * filled,
                                        out=4 * C * slots),
               atomics_bwd=dict(issued=pairs * 3 * C, per_slot_vertex_channel=filled * 3 * C, tile_face_pairs=pairs))
    for k in ("fwd", "fwd_bwd"):
        t = res[k]
        if "ms" in t["op"] and "ms" in t["torch"]:
            t["torch_over_op"] = round(t["torch"]["ms"] / t["op"]["ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg4", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interpolate_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="interpolate_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
    with torch.no_grad():
        ids, _, bary, _ = lr.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
    out["cfg3"] = [case(lr, ids, bary, ts.faces, ts.verts.shape[0], C, a.reps, a.warmup) for C in (3, 16)]
    del lr, ts, ids, bary
    torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        with torch.no_grad():
            ids, _, bary, _ = r.rasterize([0], sc.verts, sc.faces, 4)
        out["cfg4"] = [case(r, ids, bary, sc.faces, sc.verts.shape[0], C, a.reps, a.warmup) for C in (3, 16)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
