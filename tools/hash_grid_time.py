"""Time Renderer.hash_grid (dm2_hash_grid + dm2_hash_grid_backward) next to the plain-torch
encoding a user would write (``torch_encoding`` below: per level the index arithmetic, eight gathers and a weighted sum, with
autograd for its backward) at the same slots: forward under no_grad and forward + backward (the table and the position both
requiring grad), N = 16, growth 1.5, 16 levels, F = 2 and 4, T = 2^15 and 2^19.  Next to it, for context only, texture3d on a
256^3 grid with C = 4.  One JSON line on stdout; every case is echoed to stderr as it completes.

    python tools/hash_grid_time.py [--reps 10] [--warmup 2] [--bwd-reps R] [--bwd-warmup W] [--skip-cfg3] [--skip-cfg4] [--log2-rows 15 19] [--features 2 4]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4) and cfg 4 (1920x1080,
1 M-face soup, L = 4).  The positions are shading_vectors' on rasterize's hits, mapped to the unit cube of the mesh's bounding
box by (position - lo) / (hi - lo).  The two candidates alternate step by step in one process on the same inputs; device
events around each step; median and the 10th / 90th percentile over --reps after --warmup.  ``agree`` is a sanity figure: the
largest difference of the two outputs over the largest output.

Byte model, ``bytes``: forward, every slot's id (4), position (12) and NL F output floats, plus per filled slot and level eight
gathered rows of F floats (``taps``: no reuse at all) or every level's table once (``table_once``, the floor); backward,
``atomics``: one float atomic per (filled slot, level, tap, feature), what the torch lines issue, against ``table_once`` atomics
when every row's contributions merged first.
``overflow`` (cfg 4 at the larger T only): per level, the mean number of distinct rows a 16 x 16 tile's layer addresses and the
share of those rows beyond the scatter's LC_SLOTS = 512 table slots, summed over the tiles: the share of rows that cannot merge
in LDS, a stand-in for the share of contributions on the overflow route.
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

N0, GROWTH, NL = 16, 1.5, 16
LC_SLOTS = 512


def level_rows(xyz, R, T):
    """(fractions (..., 3), [row of tap p + 2 q + 4 r] * 8) of a level: clamp addressing."""
    X = xyz * R - 0.5
    X0 = torch.floor(X)
    f, c0 = X - X0, X0.long()
    c = [[(c0[..., a] + d).clamp(0, R - 1) for d in (0, 1)] for a in range(3)]
    rows = []
    for k in range(8):
        i, j, kk = c[0][k & 1], c[1][(k >> 1) & 1], c[2][(k >> 2) & 1]
        rows.append((kk * R + j) * R + i if R ** 3 <= T else (i ^ (j * 2654435761) ^ (kk * 805459861)) & (T - 1))
    return f, rows


def torch_encoding(xyz, table, live, res):
    T = table.shape[1]
    outs = []
    for l, R in enumerate(res):
        f, rows = level_rows(xyz, R, T)
        acc = 0
        for k in range(8):
            pp, qq, rr = k & 1, (k >> 1) & 1, (k >> 2) & 1
            w = (f[..., 0] if pp else 1 - f[..., 0]) * (f[..., 1] if qq else 1 - f[..., 1]) * (f[..., 2] if rr else 1 - f[..., 2])
            acc = acc + w[..., None] * table[l][rows[k]]
        outs.append(acc)
    return torch.cat(outs, -1) * live


def byte_model(slots, filled, T, F):
    table = NL * T * F * 4
    per_slot = slots * (16 + 4 * NL * F)
    taps = filled * NL * 8 * F
    return dict(taps=per_slot + 4 * taps, table_once=per_slot + min(table, 4 * taps), atomics=taps, atomics_table_once=min(NL * T * F, taps))


def overflow(xyz, ids, res, T):
    B, H, W, L = ids.shape
    assert B == 1, "one view: the groups below carry no view index"
    ty = torch.arange(H, device=ids.device) // 16
    tx = torch.arange(W, device=ids.device) // 16
    group = ((ty[:, None] * ((W + 15) // 16) + tx[None, :])[None, :, :, None] * L + torch.arange(L, device=ids.device)).expand(B, H, W, L)
    live = ids >= 0
    group = group[live]
    ngroups = int(group.max()) + 1
    p = xyz[live]
    out = []
    for R in res:
        _, rows = level_rows(p, R, T)
        keys = torch.unique(torch.cat([group * T + r for r in rows]))
        distinct = torch.bincount(keys // T, minlength=ngroups).double()
        used = distinct[distinct > 0]
        out.append(dict(R=R, rows_per_tile=round(float(used.mean()), 1),
                        beyond_table=round(float((used - LC_SLOTS).clamp(min=0).sum() / used.sum()), 4)))
    return out


def case(r, ids, xyz0, log2T, F, reps, warmup, bwd_reps, bwd_warmup):
    dev = ids.device
    T = 1 << log2T
    res = dm2.Renderer.hash_grid_resolutions(NL, N0, GROWTH)
    g = torch.Generator(device=dev).manual_seed(F)
    table = (torch.randn((NL, T, F), device=dev, generator=g) * 0.1).requires_grad_(True)
    xyz = xyz0.clone().requires_grad_(True)
    gout = torch.randn(tuple(ids.shape) + (NL * F,), device=dev, generator=g)
    live = (ids >= 0)[..., None]
    ours = lambda: r.hash_grid(xyz, table, ids, N0, GROWTH)
    torch_op = lambda: torch_encoding(xyz, table, live, res)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def fwd_bwd(fn):
        def run():
            table.grad = None
            xyz.grad = None
            fn().backward(gout)
        return run

    slots, filled = ids.numel(), int((ids >= 0).sum())
    with torch.no_grad():
        a, b = ours(), torch_op()
        agree = float((a - b).abs().max() / a.abs().max())
        del a, b
    out = dict(F=F, log2T=log2T, slots=slots, filled=filled, agree=float(f"{agree:.3g}"),
               fwd=alternate(dict(hash_grid=fwd(ours), torch=fwd(torch_op)), reps, warmup),
               fwd_bwd=alternate(dict(hash_grid=fwd_bwd(ours), torch=fwd_bwd(torch_op)), bwd_reps, bwd_warmup),
               bytes=byte_model(slots, filled, T, F))
    for k in ("fwd", "fwd_bwd"):
        out[k]["hash_grid_over_torch"] = round(out[k]["hash_grid"]["ms"] / out[k]["torch"]["ms"], 4)
    out["fwd"]["hash_grid_GBps"] = {k: round(out["bytes"][k] / out["fwd"]["hash_grid"]["ms"] / 1e6, 1) for k in ("taps", "table_once")}
    table.grad = None
    xyz.grad = None
    torch.cuda.empty_cache()
    print(json.dumps(out), file=sys.stderr, flush=True)                   # (a case takes a while on the torch side: progress)
    return out


def volume_context(r, ids, xyz0, reps, warmup):
    """texture3d at 256^3, C = 4, on the same slots: what the dense grid costs, for context."""
    dev = ids.device
    grid = torch.randn((256, 256, 256, 4), device=dev).requires_grad_(True)
    xyz = xyz0.clone().requires_grad_(True)
    gout = torch.randn(tuple(ids.shape) + (4,), device=dev)

    def fwd():
        with torch.no_grad():
            return r.texture3d(xyz, grid, ids)

    def fwd_bwd():
        grid.grad = None
        xyz.grad = None
        r.texture3d(xyz, grid, ids).backward(gout)
    res = alternate(dict(fwd=fwd, fwd_bwd=fwd_bwd), reps, warmup)
    return dict(N=256, C=4, fwd=res["fwd"], fwd_bwd=res["fwd_bwd"])


def cases(r, ids, t, verts, a, with_overflow):
    with torch.no_grad():
        pos = r.shading_vectors([0], ids, t)[0]
        lo, hi = verts.min(0).values, verts.max(0).values
        xyz = ((pos - lo) / (hi - lo)).contiguous()
    out = dict(hash_grid=[case(r, ids, xyz, log2T, F, a.reps, a.warmup, a.bwd_reps or a.reps, a.warmup if a.bwd_warmup is None else a.bwd_warmup) for log2T in a.log2_rows for F in a.features],
               texture3d=volume_context(r, ids, xyz, a.reps, a.warmup))
    if with_overflow:
        T = 1 << max(a.log2_rows)
        with torch.no_grad():
            out["overflow"] = dict(log2T=max(a.log2_rows), levels=overflow(xyz, ids, dm2.Renderer.hash_grid_resolutions(NL, N0, GROWTH), T))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bwd-reps", type=int, default=None, help="steps of the forward + backward pair (the torch side takes seconds per step); default --reps")
    ap.add_argument("--bwd-warmup", type=int, default=None, help="default --warmup")
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--log2-rows", type=int, nargs="+", default=[15, 19], help="log2 of the table's rows per level")
    ap.add_argument("--features", type=int, nargs="+", default=[2, 4], help="features per row")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hash_grid_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="hash_grid_time", reps=a.reps, warmup=a.warmup, bwd_reps=a.bwd_reps or a.reps,
               bwd_warmup=a.warmup if a.bwd_warmup is None else a.bwd_warmup, device=torch.cuda.get_device_name(0), N=N0, growth=GROWTH, NL=NL)
    if not a.skip_cfg3:
        ts = scenes.tet_lattice(1024, 1024, 25, seed=scenes.SEED_BASE + 3).to(dev)
        lr = dm2.LayeredRenderer(ts.mv, ts.proj, 1024, 1024, dev)
        with torch.no_grad():
            ids, _, _, t = lr.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
        out["cfg3"] = cases(lr, ids, t, ts.verts, a, False)
        del lr, ts, ids, t
        torch.cuda.empty_cache()
    if not a.skip_cfg4:
        sc = scenes.triangle_soup(1920, 1080, 1_000_000, scenes.SEED_BASE + 4).to(dev)
        r = dm2.Renderer(sc.mv, sc.proj, 1920, 1080, dev)
        with torch.no_grad():
            ids, _, _, t = r.rasterize([0], sc.verts, sc.faces, 4)
        out["cfg4"] = cases(r, ids, t, sc.verts, a, True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
