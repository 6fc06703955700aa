"""Time Renderer.texture (dm2_texture + dm2_texture_backward) next to the torch lines a user would write instead,

    grid = (2 * uv - 1).reshape(B, H, W * L, 2)
    out = grid_sample(tex.permute(2, 0, 1)[None].expand(B, -1, -1, -1), grid, mode="bilinear", padding_mode="border",
                      align_corners=False).permute(0, 2, 3, 1).reshape(B, H, W, L, C)

on rasterize + interpolate's output: forward under no_grad and forward + backward (tex and uv both requiring grad), clamp mode
(torch has no wrap), one texture shared by the views, C = 3 and C = 16, textures of 256^2 and 2048^2.  One JSON line.

    python tools/texture_time.py [--reps 20] [--warmup 3] [--skip-cfg4]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4) and cfg 4 (1920x1080,
1 M-face soup, L = 4).  The UV table is the planar projection of the vertices (x, y scaled to [0, 1] over the mesh's bounding
box), so the frame spans the texture about once: the 256^2 texture is magnified (several pixels per texel), the 2048^2 one is
not.  The op and the torch lines alternate step by step in one process on the same inputs; device events around each step;
median and the 10th / 90th percentile over --reps after --warmup.  Where the torch lines run out of memory the point says so
instead of a time.  Next to the times: the samples, and the global atomics of the tex backward -- one per (16 x 16 tile,
layer, texel) triple and channel if every texel finds a slot of the table (``tile_texel_pairs`` x C; the share of (tile,
layer) pairs that address more texels than the table holds is ``tiles_over_table``) against samples x 4 x C.
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

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


def torch_lines(uv, tex, ids):
    B, H, W, L, _ = uv.shape
    grid = (2 * uv - 1).reshape(B, H, W * L, 2)
    out = Fn.grid_sample(tex.permute(2, 0, 1)[None].expand(B, -1, -1, -1), grid, mode="bilinear", padding_mode="border",
                         align_corners=False)
    return out.permute(0, 2, 3, 1).reshape(B, H, W, L, tex.shape[-1])


def table_slots():
    src = open(os.path.join(ROOT, "dmesh2_renderer_amd", "csrc", "dm2_face_table.h")).read()
    return int(re.search(r"constexpr int LC_SLOTS = (\d+);", src).group(1))


def tile_texel_pairs(uv, ids, Ht, Wt):
    """(distinct (16 x 16 tile, layer, texel) triples over the four clamp-addressed corners of the filled slots -- the table is
    flushed per layer --, share of the (tile, layer) pairs with more distinct texels than the scatter's table has slots)."""
    B, H, W, L, _ = uv.shape
    x, y = uv[..., 0] * Wt - 0.5, uv[..., 1] * Ht - 0.5
    i0, j0 = torch.floor(x).long(), torch.floor(y).long()
    ys = torch.arange(H, device=uv.device).view(1, H, 1, 1) // 16
    xs = torch.arange(W, device=uv.device).view(1, 1, W, 1) // 16
    bs = torch.arange(B, device=uv.device).view(B, 1, 1, 1)
    ls = torch.arange(L, device=uv.device).view(1, 1, 1, L)
    tile = ((((bs * ((H + 15) // 16) + ys) * ((W + 15) // 16) + xs) * L + ls).expand(B, H, W, L))[ids >= 0]
    keys = []
    for dj in (0, 1):
        for di in (0, 1):
            t = (j0 + dj).clamp(0, Ht - 1) * Wt + (i0 + di).clamp(0, Wt - 1)
            keys.append(tile * (Ht * Wt) + t[ids >= 0])
    pairs = torch.unique(torch.cat(keys))
    per_tile = torch.unique(pairs // (Ht * Wt), return_counts=True)[1]
    return int(pairs.numel()), round(float((per_tile > table_slots()).float().mean()), 4)


def case(r, ids, uv0, size, C, reps, warmup):
    dev = ids.device
    g = torch.Generator(device=dev).manual_seed(C)
    tex = torch.randn((size, size, C), device=dev, generator=g).requires_grad_(True)
    uv = uv0.clone().requires_grad_(True)
    gout = torch.randn(tuple(ids.shape) + (C,), device=dev, generator=g)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(uv, tex, ids)
        return run

    def fwd_bwd(fn):
        def run():
            tex.grad = None
            uv.grad = None
            fn(uv, tex, ids).backward(gout)
        return run

    op = lambda u, t, i: r.texture(u, t, i, boundary_mode="clamp")
    slots, filled = ids.numel(), int((ids >= 0).sum())
    pairs, over = tile_texel_pairs(uv0, ids, size, size)
    res = dict(C=C, texture=size, slots=slots, filled=filled,
               fwd=alternate(dict(op=fwd(op), torch=fwd(torch_lines)), reps, warmup),
               fwd_bwd=alternate(dict(op=fwd_bwd(op), torch=fwd_bwd(torch_lines)), reps, warmup),
               atomics_bwd=dict(all_in_table=pairs * C, per_sample_corner_channel=filled * 4 * C, tile_texel_pairs=pairs,
                                tiles_over_table=over))
    for k in ("fwd", "fwd_bwd"):
        t = res[k]
        if "ms" in t["op"] and "ms" in t["torch"]:
            t["torch_over_op"] = round(t["torch"]["ms"] / t["op"]["ms"], 2)
    return res


def planar_uv(verts):
    lo, hi = verts[:, :2].min(0).values, verts[:, :2].max(0).values
    return ((verts[:, :2] - lo) / (hi - lo)).contiguous()


def cases(r, ids, bary, verts, faces, reps, warmup):
    with torch.no_grad():
        uv = r.interpolate(ids, bary, planar_uv(verts), faces)
    return [case(r, ids, uv, size, C, reps, warmup) for size in (256, 2048) for C in (3, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg4", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="texture_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
    with torch.no_grad():
        ids, _, bary, _ = lr.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
    out["cfg3"] = cases(lr, ids, bary, ts.verts, ts.faces, a.reps, a.warmup)
    del lr, ts, ids, bary
    torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        with torch.no_grad():
            ids, _, bary, _ = r.rasterize([0], sc.verts, sc.faces, 4)
        out["cfg4"] = cases(r, ids, bary, sc.verts, sc.faces, a.reps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
