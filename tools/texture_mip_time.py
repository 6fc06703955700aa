"""Time the mip-mapped texture path: Renderer.bary_derivatives, the two extra interpolate calls that turn its outputs into the UV
footprint, Renderer.texture_mipmaps and its backward, and Renderer.texture in "linear" against "linear-mipmap-linear", forward
under no_grad and forward + backward (tex, mip and uv requiring grad; the chain handed in, so that its own backward is timed on
its own).  One JSON line.

    python tools/texture_mip_time.py [--reps 20] [--warmup 3] [--repeat 4] [--skip-cfg3] [--skip-cfg4]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4) and cfg 4 (1920x1080,
1 M-face soup, L = 4).  A 2048^2 texture, C = 3 and C = 16, wrap mode.  The UV table is the planar projection of the vertices
scaled so that the frame spans the texture ``--repeat`` times (default 4): about 8 texels per pixel on cfg 3, so most slots are
minified (``levels``: the share of the filled slots whose first level is k; ``magnified``: lod <= 0).  The steps alternate
round-robin in one process on the same inputs; device events around each step; median and the 10th / 90th percentile over
--reps after --warmup.  ``bytes``: what each step must move at least (the byte model of DESIGN.md 8), ``GBps`` = bytes / median.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import dmesh2_renderer_amd as dm2  # noqa: E402
from dmesh2_renderer_amd import _C, scenes  # noqa: E402
from texture_time import alternate, planar_uv  # noqa: E402

MODE = "linear-mipmap-linear"
SIZE = 2048


def level_shares(uv_da, ids, size):
    """(share of the filled slots with lod <= 0, [share whose first level is k]) from the exact 0.5 log2 (a description of the
    workload, not the op's own bits)."""
    d = uv_da[ids >= 0].double() * size
    r2 = torch.maximum(d[:, 0] ** 2 + d[:, 1] ** 2, d[:, 2] ** 2 + d[:, 3] ** 2)
    r2 = r2[torch.isfinite(r2)]
    lod = 0.5 * torch.log2(r2.clamp(min=1.0))
    nlev = _C.mip_layout(size, size)[0]
    j = lod.floor().clamp(max=nlev - 1).long()
    return round(float((lod <= 0).double().mean()), 4), [round(float((j == k).double().mean()), 4) for k in range(nlev)]


def case(r, ids, uv0, uv_da, C, reps, warmup):
    dev = ids.device
    g = torch.Generator(device=dev).manual_seed(C)
    tex = torch.randn((SIZE, SIZE, C), device=dev, generator=g).requires_grad_(True)
    with torch.no_grad():
        mip0 = r.texture_mipmaps(tex)
    mip = mip0.clone().requires_grad_(True)
    uv = uv0.clone().requires_grad_(True)
    gout = torch.randn(tuple(ids.shape) + (C,), device=dev, generator=g)
    gmip = torch.randn(tuple(mip0.shape), device=dev, generator=g)

    def clear():
        tex.grad = None
        mip.grad = None
        uv.grad = None

    def linear_fwd():
        with torch.no_grad():
            r.texture(uv, tex, ids)

    def mip_fwd():
        with torch.no_grad():
            r.texture(uv, tex, ids, MODE, uv_da=uv_da, mip=mip)

    def linear_fwd_bwd():
        clear()
        r.texture(uv, tex, ids).backward(gout)

    def mip_fwd_bwd():
        clear()
        r.texture(uv, tex, ids, MODE, uv_da=uv_da, mip=mip).backward(gout)

    def chain_fwd():
        with torch.no_grad():
            r.texture_mipmaps(tex)

    def chain_fwd_bwd():
        clear()
        r.texture_mipmaps(tex).backward(gmip)

    slots, filled = ids.numel(), int((ids >= 0).sum())
    texels, T = SIZE * SIZE, _C.mip_layout(SIZE, SIZE)[2]
    res = dict(C=C, texture=SIZE, slots=slots, filled=filled,
               times=alternate(dict(linear_fwd=linear_fwd, mip_fwd=mip_fwd, linear_fwd_bwd=linear_fwd_bwd, mip_fwd_bwd=mip_fwd_bwd,
                                    chain_fwd=chain_fwd, chain_fwd_bwd=chain_fwd_bwd), reps, warmup))
    # the least each step moves: ids + uv (+ uv_da) in, C floats out per slot (texels from cache); the chain reads tex and writes
    # T texels, its backward reads T and writes the texture
    res["bytes"] = dict(linear_fwd=slots * (4 + 8 + 4 * C), mip_fwd=slots * (4 + 8 + 16 + 4 * C), chain_fwd=4 * C * (texels + T),
                        chain_bwd=4 * C * (texels + T))
    t = res["times"]
    for k in ("linear_fwd", "mip_fwd", "chain_fwd"):
        if "ms" in t[k]:
            t[k]["GBps"] = round(res["bytes"][k] / t[k]["ms"] / 1e6, 1)
    if "ms" in t["chain_fwd"] and "ms" in t["chain_fwd_bwd"]:
        bwd = t["chain_fwd_bwd"]["ms"] - t["chain_fwd"]["ms"]
        t["chain_bwd"] = dict(ms=round(bwd, 4), GBps=round(res["bytes"]["chain_bwd"] / max(bwd, 1e-6) / 1e6, 1))
    for a, b in (("mip_fwd", "linear_fwd"), ("mip_fwd_bwd", "linear_fwd_bwd")):
        if "ms" in t[a] and "ms" in t[b]:
            res[a + "_over_" + b] = round(t[a]["ms"] / t[b]["ms"], 3)
    return res


def cases(r, idx, ids, bary, verts, faces, repeat, reps, warmup):
    table = planar_uv(verts) * repeat
    with torch.no_grad():
        uv = r.interpolate(ids, bary, table, faces)
        dx, dy = r.bary_derivatives(idx, ids, verts, faces)
        uv_da = torch.cat([r.interpolate(ids, dx, table, faces), r.interpolate(ids, dy, table, faces)], -1)

    def footprint():
        with torch.no_grad():
            r.bary_derivatives(idx, ids, verts, faces)

    def interpolate_twice():
        with torch.no_grad():
            r.interpolate(ids, dx, table, faces)
            r.interpolate(ids, dy, table, faces)

    slots = ids.numel()
    prep = alternate(dict(bary_derivatives=footprint, interpolate_x2=interpolate_twice), reps, warmup)
    # per slot: the id in, two 12-byte rows out (the face's row and its three vertices mostly from cache)
    if "ms" in prep["bary_derivatives"]:
        prep["bary_derivatives"]["GBps"] = round(slots * (4 + 24) / prep["bary_derivatives"]["ms"] / 1e6, 1)
    magnified, levels = level_shares(uv_da, ids, SIZE)
    return dict(repeat=repeat, magnified=magnified, levels=levels, footprint=prep,
                texture=[case(r, ids, uv, uv_da, C, reps, warmup) for C in (3, 16)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=float, default=4.0)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--skip-cfg4", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_mip_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="texture_mip_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    if not a.skip_cfg3:
        ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
        lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
        with torch.no_grad():
            ids, _, bary, _ = lr.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
        out["cfg3"] = cases(lr, [0], ids, bary, ts.verts, ts.faces, a.repeat, a.reps, a.warmup)
        del lr, ts, ids, bary
        torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        with torch.no_grad():
            ids, _, bary, _ = r.rasterize([0], sc.verts, sc.faces, 4)
        out["cfg4"] = cases(r, [0], ids, bary, sc.verts, sc.faces, a.repeat, a.reps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
