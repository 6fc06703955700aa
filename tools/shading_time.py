"""Time Renderer.vertex_normals and Renderer.shading_vectors next to the torch lines they replace.  One JSON line.

    python tools/shading_time.py [--reps 20] [--warmup 3] [--skip-cfg3] [--skip-cfg4]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags) and cfg 4 (1920x1080, 1 M-face
soup), L = 4.  The candidates of a comparison alternate step by step in one process on the same inputs; device events around
each step; median and the 10th / 90th percentile over --reps after --warmup.

vertex_normals: ``hip`` is r.vertex_normals(verts, faces, adjacency) with the adjacency prebuilt (``adjacency_build`` times
Renderer.vertex_adjacency alone: once per topology, not per step); ``torch`` is tools/texture_cube_time.py's line (a cross
product and three index_add_) plus torch.nn.functional.normalize.  fwd under no_grad, fwd_bwd with verts requiring grad and a
dense upstream gradient.  Byte model (``bytes``), compulsory traffic with every gather counted once per use:
  fwd  faces 12 F + vertex gathers 36 F + face rows written 16 F | offsets 4 P + corners 12 F + rows gathered 48 F + out and len 16 P
  bwd  faces 12 F + vertex gathers 36 F + double face rows written 32 F | g, n, len 28 P + offsets 4 P + corners 12 F + double
       rows gathered 96 F + d rows 16 P | faces 12 F + vertex and d gathers 84 F + corner rows written 48 F | offsets 4 P +
       corners 12 F + rows gathered 48 F + dverts 12 P

shading_vectors: ``hip`` is r.shading_vectors(idx, layers, t, normals) with normals; ``torch`` the broadcast and the
elementwise lines a caller writes with ray tensors: position = ro + t rd, view = -rd, normal = normalize(n), reflection =
2 (normal . view) normal - view, each masked by the slot's id.  fwd under no_grad, fwd_bwd with t and normals requiring grad
and dense upstream gradients on position, normal and reflection.  Byte model per slot: fwd 8 (id, t) + 12 (normal) + 24 / L
(the ray, shared by the pixel's slots) read, 48 written; bwd the same reads + 36 (three upstream rows), 16 written.
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


def torch_normals(verts, faces_long):
    a, b, c = verts[faces_long[:, 0]], verts[faces_long[:, 1]], verts[faces_long[:, 2]]
    fn = torch.cross(b - a, c - a, dim=-1)
    n = torch.zeros_like(verts)
    for k in range(3):
        n = n.index_add(0, faces_long[:, k], fn)
    return torch.nn.functional.normalize(n, dim=-1)


def torch_shading(layers, t, normals, ray_o, ray_d):
    live = (layers >= 0)[..., None]
    ro, rd = ray_o[:, :, :, None, :], ray_d[:, :, :, None, :]
    position = torch.where(live, ro + t[..., None] * rd, 0.0)
    view = torch.where(live, -rd, 0.0)
    normal = torch.where(live, torch.nn.functional.normalize(normals, dim=-1), 0.0)
    reflection = 2.0 * (normal * view).sum(-1, keepdim=True) * normal - view
    return position, view, normal, reflection


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def normals_case(r, verts0, faces, reps, warmup):
    P, F = verts0.shape[0], faces.shape[0]
    fl = faces.long()
    adjacency = r.vertex_adjacency(faces, P)
    verts = verts0.clone().requires_grad_(True)
    g = torch.randn((P, 3), device=verts.device, generator=torch.Generator(device=verts.device).manual_seed(1))
    hip = lambda: r.vertex_normals(verts, faces, adjacency)
    ref = lambda: torch_normals(verts, fl)

    def fwd_bwd(fn):
        def run():
            verts.grad = None
            fn().backward(g)
        return run

    with torch.no_grad():
        agree = float((hip() - ref()).abs().max())
    res = dict(P=P, F=F, max_abs_diff=agree,
               adjacency_build=alternate(dict(build=lambda: r.vertex_adjacency(faces, P)), reps, warmup)["build"],
               fwd=alternate(dict(hip=no_grad(hip), torch=no_grad(ref)), reps, warmup),
               fwd_bwd=alternate(dict(hip=fwd_bwd(hip), torch=fwd_bwd(ref)), reps, warmup),
               bytes=dict(fwd=64 * F + 4 * P + 60 * F + 16 * P, bwd=80 * F + 48 * P + 108 * F + 144 * F + 16 * P + 60 * F))
    for k in ("fwd", "fwd_bwd"):
        res[k]["hip_over_torch"] = round(res[k]["hip"]["ms"] / res[k]["torch"]["ms"], 3)
    res["fwd"]["hip_GBps"] = round(res["bytes"]["fwd"] / res["fwd"]["hip"]["ms"] / 1e6, 1)
    res["fwd_bwd"]["hip_GBps"] = round((res["bytes"]["fwd"] + res["bytes"]["bwd"]) / res["fwd_bwd"]["hip"]["ms"] / 1e6, 1)
    return res


def shading_case(r, idx, layers, t0, normals0, reps, warmup):
    dev = layers.device
    gen = torch.Generator(device=dev).manual_seed(2)
    gs = [torch.randn(tuple(layers.shape) + (3,), device=dev, generator=gen) for _ in range(3)]
    t, normals = t0.clone().requires_grad_(True), normals0.clone().requires_grad_(True)
    ray_o, ray_d = r._camera_rows(r.ray_o, idx), r._camera_rows(r.ray_d, idx)
    hip = lambda: r.shading_vectors(idx, layers, t, normals)
    ref = lambda: torch_shading(layers, t, normals, ray_o, ray_d)

    def fwd_bwd(fn):
        def run():
            t.grad = normals.grad = None
            p, _, n, rf = fn()
            torch.autograd.backward((p, n, rf), gs)
        return run

    with torch.no_grad():
        agree = max(float((a - b).abs().max()) for a, b in zip(hip(), ref()))
    S, L = layers.numel(), layers.shape[-1]
    res = dict(slots=S, filled=int((layers >= 0).sum()), L=L, max_abs_diff=agree,
               fwd=alternate(dict(hip=no_grad(hip), torch=no_grad(ref)), reps, warmup),
               fwd_bwd=alternate(dict(hip=fwd_bwd(hip), torch=fwd_bwd(ref)), reps, warmup),
               bytes=dict(fwd=S * (20 + 48) + S // L * 24, bwd=S * (20 + 36 + 16) + S // L * 24))
    for k in ("fwd", "fwd_bwd"):
        res[k]["hip_over_torch"] = round(res[k]["hip"]["ms"] / res[k]["torch"]["ms"], 3)
    res["fwd"]["hip_GBps"] = round(res["bytes"]["fwd"] / res["fwd"]["hip"]["ms"] / 1e6, 1)
    res["fwd_bwd"]["hip_GBps"] = round((res["bytes"]["fwd"] + res["bytes"]["bwd"]) / res["fwd_bwd"]["hip"]["ms"] / 1e6, 1)
    return res


def config(r, verts, faces, faces_existence, a):
    with torch.no_grad():
        layers, _, bary, t = r.rasterize([0], verts, faces, 4, faces_existence=faces_existence)
        normals = r.interpolate(layers, bary, r.vertex_normals(verts, faces), faces)
    return dict(vertex_normals=normals_case(r, verts, faces, a.reps, a.warmup),
                shading_vectors=shading_case(r, [0], layers, t, normals, a.reps, a.warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--skip-cfg4", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shading_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="shading_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    if not a.skip_cfg3:
        ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
        lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
        out["cfg3"] = config(lr, ts.verts, ts.faces, ts.faces_existence, a)
        del lr, ts
        torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        out["cfg4"] = config(r, sc.verts, sc.faces, None, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
