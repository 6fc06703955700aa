"""Time Renderer.texture(boundary_mode="cube") (dm2_texture_cube + dm2_texture_cube_backward) next to the 2D op on an atlas,

    out = r.texture(atlas_uv, atlas, ids, "linear", "clamp")          # atlas (N, 6 N, C): the six faces side by side

at the same slots and C: forward under no_grad and forward + backward (the texture and the lookup coordinate both requiring
grad), one cube shared by the views, C = 3 and C = 16, faces of 64^2 and 1024^2.  One JSON line.

    python tools/texture_cube_time.py [--reps 20] [--warmup 3] [--skip-cfg3] [--skip-cfg4] [--faces 64 1024]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4) and cfg 4 (1920x1080,
1 M-face soup, L = 4).  The directions are the area-weighted vertex normals of the mesh, interpolated on rasterize's hits
and normalised.  The atlas lookup filters wrongly across every edge -- it is not an alternative, it is the yardstick: the same
four taps per sample from a texture of the same size, so its byte model differs from the cube's by one float per slot (a
direction has three components, a uv two).  The atlas uv is ((face + s) / 6, t) of the cube's own face and face coordinates,
computed beforehand (not timed).  The two ops alternate step by step in one process on the same inputs; device events around
each step; median and the 10th / 90th percentile over --reps after --warmup.  ``same_as_atlas`` is a sanity figure: the share
of filled slots where the two outputs agree within 1e-4 (they differ at the seams, and on large faces everywhere, where the
atlas' u = (face + s) / 6 has lost the low bits of s).

Byte model per call, ``bytes``: every slot's id (4), lookup coordinate (12 or 8) and C output floats, plus the texels:
``tex_once`` counts the texture once (the floor when it is reused from cache: 6 N N C floats, or the taps if fewer),
``tex_taps`` four taps of C floats per filled slot (no reuse at all).  The backward adds the upstream gradient and the
coordinate's gradient per slot, the texture read again for the coordinate's gradient, and the texel scatter.
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


def vertex_normals(verts, faces):
    """Area-weighted vertex normals (the sum of the cross products of the faces round a vertex), not normalised."""
    f = faces.long()
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    fn = torch.cross(b - a, c - a, dim=-1)
    n = torch.zeros_like(verts)
    for k in range(3):
        n.index_add_(0, f[:, k], fn)
    return n


def atlas_uv(dirs):
    """((face + s) / 6, t) of each direction by the cube's own rules (include/dm2_hip.h: dm2_texture_cube); zero directions
    give (0, 0): their slots are empty by id."""
    x, y, z = dirs.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    is_x = (ax >= ay) & (ax >= az)
    is_y = ~is_x & (ay >= az)
    major = torch.where(is_x, x, torch.where(is_y, y, z))
    neg = major < 0
    face = torch.where(is_x, 0, torch.where(is_y, 2, 4)) + neg.long()
    ma = major.abs().clamp_min(1e-30)
    sc = torch.where(is_x, torch.where(neg, z, -z), torch.where(is_y, x, torch.where(neg, -x, x)))
    tc = torch.where(is_y, torch.where(neg, -z, z), -y)
    s, t = 0.5 * (sc / ma + 1), 0.5 * (tc / ma + 1)
    return torch.stack([(face + s) / 6, t], -1).contiguous()


def byte_model(slots, filled, N, C, coord):
    texture = 6 * N * N * C * 4
    taps = filled * 4 * C * 4
    per_slot_fwd = slots * (4 + 4 * coord + 4 * C)
    per_slot_bwd = slots * (4 + 4 * coord + 4 * C) * 2 + slots * 4 * coord        # the two backward kernels read ids, coordinates and g
    return dict(fwd=dict(tex_once=per_slot_fwd + min(texture, taps), tex_taps=per_slot_fwd + taps),
                bwd=dict(tex_once=per_slot_bwd + 2 * min(texture, taps), tex_taps=per_slot_bwd + 2 * taps))


def case(r, ids, dirs0, uv0, N, C, reps, warmup):
    dev = ids.device
    g = torch.Generator(device=dev).manual_seed(C)
    cube = torch.randn((6, N, N, C), device=dev, generator=g).requires_grad_(True)
    atlas = cube.detach().permute(1, 0, 2, 3).reshape(N, 6 * N, C).contiguous().requires_grad_(True)
    dirs, uv = dirs0.clone().requires_grad_(True), uv0.clone().requires_grad_(True)
    gout = torch.randn(tuple(ids.shape) + (C,), device=dev, generator=g)
    cube_op = lambda: r.texture(dirs, cube, ids, boundary_mode="cube")
    atlas_op = lambda: r.texture(uv, atlas, ids, boundary_mode="clamp")

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def fwd_bwd(fn, leaves):
        def run():
            for x in leaves:
                x.grad = None
            fn().backward(gout)
        return run

    slots, filled = ids.numel(), int((ids >= 0).sum())
    with torch.no_grad():
        inside = float(((cube_op() - atlas_op()).abs().amax(-1) <= 1e-4)[ids >= 0].float().mean())
    res = dict(C=C, N=N, slots=slots, filled=filled, same_as_atlas=round(inside, 4),
               fwd=alternate(dict(cube=fwd(cube_op), atlas2d=fwd(atlas_op)), reps, warmup),
               fwd_bwd=alternate(dict(cube=fwd_bwd(cube_op, (cube, dirs)), atlas2d=fwd_bwd(atlas_op, (atlas, uv))), reps, warmup),
               bytes=dict(cube=byte_model(slots, filled, N, C, 3), atlas2d=byte_model(slots, filled, N, C, 2)))
    for k in ("fwd", "fwd_bwd"):
        res[k]["cube_over_atlas2d"] = round(res[k]["cube"]["ms"] / res[k]["atlas2d"]["ms"], 3)
    b = res["bytes"]["cube"]["fwd"]
    res["fwd"]["cube_GBps"] = dict(tex_once=round(b["tex_once"] / res["fwd"]["cube"]["ms"] / 1e6, 1),
                                   tex_taps=round(b["tex_taps"] / res["fwd"]["cube"]["ms"] / 1e6, 1))
    return res


def cases(r, ids, bary, verts, faces, a):
    with torch.no_grad():
        dirs = torch.nn.functional.normalize(r.interpolate(ids, bary, vertex_normals(verts, faces), faces), dim=-1)
        uv = atlas_uv(dirs)
    return [case(r, ids, dirs, uv, N, C, a.reps, a.warmup) for N in a.faces for C in (3, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--faces", type=int, nargs="+", default=[64, 1024], help="face sizes N (one per process under a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_cube_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="texture_cube_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
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
