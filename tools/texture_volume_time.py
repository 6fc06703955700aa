"""Time Renderer.texture3d (dm2_texture_volume + dm2_texture_volume_backward) next to the lines it
replaces,

    vol = grid.permute(3, 0, 1, 2)[None]                                  # channel-first, as grid_sample wants it
    out = torch.nn.functional.grid_sample(vol, 2 * xyz - 1, "bilinear", "border", align_corners=False)
    out = out[0].permute(1, 2, 3, 0) * (ids >= 0)[..., None]              # channel-last again, empty slots zeroed

at the same slots and C: forward under no_grad and forward + backward (the grid and the position both requiring grad), one
grid shared by the view, C = 3, 4 and 16, grids of 64^3 and 256^3.  One JSON line.

    python tools/texture_volume_time.py [--reps 20] [--warmup 3] [--skip-cfg3] [--skip-cfg4] [--grids 64 256]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4) and cfg 4 (1920x1080,
1 M-face soup, L = 4).  The positions are shading_vectors' on rasterize's hits, mapped to the unit cube of the mesh's bounding
box by (position - lo) / (hi - lo).  The two candidates alternate step by step in one process on the same inputs; device
events around each step; median and the 10th / 90th percentile over --reps after --warmup.  ``agree`` is a sanity figure: the
largest difference of the two outputs over the largest output.

Byte model per forward call, ``bytes``: every slot's id (4), position (12) and C output floats, plus the voxels: ``grid_once``
counts the grid once (the floor when it is reused from cache: N^3 C floats, or the taps if fewer), ``grid_taps`` eight gathered
rows of C floats per filled slot (no reuse at all).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import dmesh2_renderer_amd as dm2  # noqa: E402
from dmesh2_renderer_amd import scenes  # noqa: E402
from texture_cube_time import alternate  # noqa: E402


def byte_model(slots, filled, N, C):
    grid = N * N * N * C * 4
    taps = filled * 8 * C * 4
    per_slot = slots * (16 + 4 * C)
    return dict(grid_once=per_slot + min(grid, taps), grid_taps=per_slot + taps)


def case(r, ids, xyz0, N, C, reps, warmup):
    dev = ids.device
    g = torch.Generator(device=dev).manual_seed(C)
    grid = torch.randn((N, N, N, C), device=dev, generator=g).requires_grad_(True)
    xyz = xyz0.clone().requires_grad_(True)
    gout = torch.randn(tuple(ids.shape) + (C,), device=dev, generator=g)
    live = (ids >= 0)[..., None]
    ours = lambda: r.texture3d(xyz, grid, ids)

    def torch_op():
        vol = grid.permute(3, 0, 1, 2)[None].expand(xyz.shape[0], -1, -1, -1, -1)
        out = torch.nn.functional.grid_sample(vol, 2.0 * xyz - 1.0, mode="bilinear", padding_mode="border", align_corners=False)
        return out.permute(0, 2, 3, 4, 1) * live

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def fwd_bwd(fn):
        def run():
            grid.grad = None
            xyz.grad = None
            fn().backward(gout)
        return run

    slots, filled = ids.numel(), int((ids >= 0).sum())
    with torch.no_grad():
        a, b = ours(), torch_op()
        agree = float((a - b).abs().max() / a.abs().max())
    res = dict(C=C, N=N, slots=slots, filled=filled, agree=float(f"{agree:.3g}"),
               fwd=alternate(dict(texture3d=fwd(ours), grid_sample=fwd(torch_op)), reps, warmup),
               fwd_bwd=alternate(dict(texture3d=fwd_bwd(ours), grid_sample=fwd_bwd(torch_op)), reps, warmup),
               bytes=byte_model(slots, filled, N, C))
    for k in ("fwd", "fwd_bwd"):
        res[k]["texture3d_over_grid_sample"] = round(res[k]["texture3d"]["ms"] / res[k]["grid_sample"]["ms"], 3)
    res["fwd"]["texture3d_GBps"] = {k: round(v / res["fwd"]["texture3d"]["ms"] / 1e6, 1) for k, v in res["bytes"].items()}
    return res


def cases(r, ids, t, verts, a):
    with torch.no_grad():
        pos = r.shading_vectors([0], ids, t)[0]
        lo, hi = verts.min(0).values, verts.max(0).values
        xyz = ((pos - lo) / (hi - lo)).contiguous()
    return [case(r, ids, xyz, N, C, a.reps, a.warmup) for N in a.grids for C in (3, 4, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--grids", type=int, nargs="+", default=[64, 256], help="grid sizes N")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_volume_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="texture_volume_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    if not a.skip_cfg3:
        ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
        lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
        with torch.no_grad():
            ids, _, _, t = lr.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
        out["cfg3"] = cases(lr, ids, t, ts.verts, a)
        del lr, ts, ids, t
        torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        with torch.no_grad():
            ids, _, _, t = r.rasterize([0], sc.verts, sc.faces, 4)
        out["cfg4"] = cases(r, ids, t, sc.verts, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
