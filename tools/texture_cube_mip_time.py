"""Time Renderer.texture(..., "linear-mipmap-linear", "cube", mip=chain, mip_level=level) (dm2_texture_cube_mip /
dm2_texture_cube_mip_backward) next to

  per_level   the route without the op: one "linear" cube call per level over all slots, a torch gather of the two levels
              round each slot's level and a lerp, with autograd (nlev scatters in the backward);
  linear      one "linear" cube call on the same slots: a yardstick, not a bar.

Forward under no_grad and forward + backward (the cube, its chain, the directions and the level all requiring grad; for
``linear`` the cube and the directions), one cube shared by the views, C = 3 and C = 16, faces of 64^2 and 1024^2, the levels
of the slots spread evenly over [0, nlev - 1].  One JSON line.

    python tools/texture_cube_mip_time.py [--reps 20] [--warmup 3] [--skip-cfg3] [--skip-cfg4] [--faces 64 1024]

Scenes and directions: tools/texture_cube_time.py's (cfg 3, cfg 4, L = 4; the mesh's area-weighted normals on rasterize's
hits).  The candidates alternate step by step in one process on the same inputs; device events round each step; median and
the 10th / 90th percentile over --reps after --warmup.

Byte model per forward call, ``bytes``: every slot's id (4), direction (12), level (4) and C output floats, plus the texels:
a slot between two levels reads eight taps of C floats where ``linear`` reads four, so with no reuse at all the op moves
(20 + 4 C + 32 C) / (16 + 4 C + 16 C) of ``linear``'s bytes per filled slot: 1.71 at C = 3, 1.77 at C = 16; towards 2 as C
grows, and below that where the coarse levels stay in cache (their texels are few).  ``op_over_linear`` is the measured ratio.
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
from dmesh2_renderer_amd import _C, scenes  # noqa: E402
from texture_cube_time import alternate, vertex_normals  # noqa: E402


def level_cubes(tex, mip, N):
    """[level 0 .. nlev-1] as cubes (6, N_k, N_k, C): views of tex and of the packed chain."""
    nlev, levels, _ = _C.mip_layout(N, N)
    return [tex] + [mip[:, off:off + n * n].reshape(6, n, n, tex.shape[-1]) for n, _, off in levels[1:]]


def per_level_route(r, dirs, tex, mip, ids, level, N):
    nlev = _C.mip_layout(N, N)[0]
    c = torch.stack([r.texture(dirs, lv, ids, boundary_mode="cube") for lv in level_cubes(tex, mip, N)], 0)     # (nlev,B,H,W,L,C)
    lod = level.clamp(0, nlev - 1)
    j = lod.floor().clamp(max=max(nlev - 2, 0)).long()
    f = (lod - j)[..., None]
    pick = lambda k: torch.gather(c, 0, k[None, ..., None].expand((1,) + tuple(c.shape[1:])))[0]
    cj = pick(j)
    return cj + f * (pick((j + 1).clamp(max=nlev - 1)) - cj)


def case(r, ids, dirs0, N, C, reps, warmup):
    dev = ids.device
    g = torch.Generator(device=dev).manual_seed(C)
    nlev = _C.mip_layout(N, N)[0]
    cube = torch.randn((6, N, N, C), device=dev, generator=g).requires_grad_(True)
    mip = r.texture_mipmaps(cube.detach()).requires_grad_(True)
    dirs = dirs0.clone().requires_grad_(True)
    level = (torch.rand(tuple(ids.shape), device=dev, generator=g) * (nlev - 1)).requires_grad_(True)
    gout = torch.randn(tuple(ids.shape) + (C,), device=dev, generator=g)
    op = lambda: r.texture(dirs, cube, ids, "linear-mipmap-linear", "cube", mip=mip, mip_level=level)
    route = lambda: per_level_route(r, dirs, cube, mip, ids, level, N)
    linear = lambda: r.texture(dirs, cube, ids, boundary_mode="cube")

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def fwd_bwd(fn):
        def run():
            for x in (cube, mip, dirs, level):
                x.grad = None
            fn().backward(gout)
        return run

    slots, filled = ids.numel(), int((ids >= 0).sum())
    with torch.no_grad():
        agree = float((op() - route()).abs().max())
    names = dict(op=op, per_level=route, linear=linear)
    res = dict(C=C, N=N, nlev=nlev, slots=slots, filled=filled, max_abs_op_minus_per_level=agree,
               fwd=alternate({k: fwd(v) for k, v in names.items()}, reps, warmup),
               fwd_bwd=alternate({k: fwd_bwd(v) for k, v in names.items()}, reps, warmup),
               bytes=dict(op=slots * (20 + 4 * C) + filled * 32 * C, linear=slots * (16 + 4 * C) + filled * 16 * C))
    res["bytes"]["op_over_linear"] = round(res["bytes"]["op"] / res["bytes"]["linear"], 3)
    for k in ("fwd", "fwd_bwd"):
        res[k]["op_over_per_level"] = round(res[k]["op"]["ms"] / res[k]["per_level"]["ms"], 3)
        res[k]["op_over_linear"] = round(res[k]["op"]["ms"] / res[k]["linear"]["ms"], 3)
    return res


def cases(r, ids, bary, verts, faces, a):
    with torch.no_grad():
        dirs = torch.nn.functional.normalize(r.interpolate(ids, bary, vertex_normals(verts, faces), faces), dim=-1)
    return [case(r, ids, dirs, N, C, a.reps, a.warmup) for N in a.faces for C in (3, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--faces", type=int, nargs="+", default=[64, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_cube_mip_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="texture_cube_mip_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    if not a.skip_cfg3:
        ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
        lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
        with torch.no_grad():
            ids, _, bary, _ = lr.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
        out["cfg3"] = cases(lr, ids, bary, ts.verts, ts.faces, a)
        del lr, ts, ids, bary
        torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        with torch.no_grad():
            ids, _, bary, _ = r.rasterize([0], sc.verts, sc.faces, 4)
        out["cfg4"] = cases(r, ids, bary, sc.verts, sc.faces, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
