"""Time Renderer.composite (dm2_composite + dm2_composite_backward) next to the torch lines a user would write instead,

    a = torch.where(ids >= 0, alpha[ids.clamp(min=0)], 0)            # per-face alpha; a per-slot alpha is masked only
    trans = torch.cumprod(1 - a, -1)
    front = torch.cat([torch.ones_like(trans[..., :1]), trans[..., :-1]], -1)
    out = (values * (a * front)[..., None]).sum(-2) + trans[..., -1:] * background
    acc = 1 - trans[..., -1]

(tests/composite_ref.py: one_liner) on rasterize + interpolate's output: forward under no_grad and forward + backward (values
and alpha both requiring grad, a loss over out and acc), C = 3 and C = 16, a per-slot and a per-face alpha.  One JSON line.

    python tools/composite_time.py [--reps 20] [--warmup 3] [--skip-cfg4]

Scenes: SURVEY.md 8(d) cfg 3 (1024^2, tet_lattice(n=25), seed SEED_BASE + 3, its existence flags, L = 4) and cfg 4 (1920x1080,
1 M-face soup, L = 4).  values = interpolate of a random C-channel vertex table; opacities uniform in [0.05, 0.95] per face
(the per-slot alpha is that table gathered once, outside the timed region).  The op and the torch lines alternate step by step
in one process on the same inputs; device events around each step; median and the 10th / 90th percentile over --reps after
--warmup.  Next to the times the byte model: the bytes a call asks for if every array is touched once (forward: values, ids,
alpha in, out, acc, final_T, n_contrib out; backward: values, ids, alpha, n_contrib, g, gA in, dL/dvalues and a per-slot
dL/dalpha out) and the rate that makes at the op's median.
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


def torch_lines(values, alpha, ids, background):
    if alpha.dim() == 1:
        a = torch.where(ids >= 0, alpha[ids.clamp(min=0).long()], torch.zeros_like(values[..., 0]))
    else:
        a = torch.where(ids >= 0, alpha, torch.zeros_like(alpha))
    trans = torch.cumprod(1 - a, -1)
    front = torch.cat([torch.ones_like(trans[..., :1]), trans[..., :-1]], -1)
    out = (values * (a * front)[..., None]).sum(-2) + trans[..., -1:] * background
    return out, 1 - trans[..., -1]


def case(r, ids, values0, opacity, per_face, reps, warmup):
    dev = ids.device
    C = values0.shape[-1]
    g = torch.Generator(device=dev).manual_seed(C)
    background = torch.rand(C, device=dev, generator=g)
    alpha0 = opacity if per_face else torch.where(ids >= 0, opacity[ids.clamp(min=0).long()], torch.zeros((), device=dev))
    values, alpha = values0.clone().requires_grad_(True), alpha0.clone().requires_grad_(True)
    gout = torch.randn(tuple(ids.shape[:3]) + (C,), device=dev, generator=g)
    gacc = torch.randn(tuple(ids.shape[:3]), device=dev, generator=g)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(values, alpha, ids, background)
        return run

    def fwd_bwd(fn):
        def run():
            values.grad = None
            alpha.grad = None
            torch.autograd.backward(fn(values, alpha, ids, background), [gout, gacc])
        return run

    op = lambda v, a, i, b: r.composite(v, a, i, b)
    P, S = ids[..., 0].numel(), ids.numel()
    fwd_bytes = 4 * (S * C + 2 * S + P * C + 3 * P)
    bwd_bytes = 4 * (2 * S * C + 2 * S + P + P * C + P + (0 if per_face else S))
    res = dict(C=C, alpha="per_face" if per_face else "per_slot", pixels=P, slots=S, filled=int((ids >= 0).sum()),
               fwd=alternate(dict(op=fwd(op), torch=fwd(torch_lines)), reps, warmup),
               fwd_bwd=alternate(dict(op=fwd_bwd(op), torch=fwd_bwd(torch_lines)), reps, warmup),
               bytes=dict(fwd=fwd_bytes, fwd_bwd=fwd_bytes + bwd_bytes))
    for k in ("fwd", "fwd_bwd"):
        t = res[k]
        if "ms" in t["op"]:
            t["op_TBps"] = round(res["bytes"][k] / (t["op"]["ms"] * 1e-3) / 1e12, 3)
        if "ms" in t["op"] and "ms" in t["torch"]:
            t["torch_over_op"] = round(t["torch"]["ms"] / t["op"]["ms"], 2)
    return res


def cases(r, ids, bary, verts, faces, reps, warmup):
    dev = ids.device
    out = []
    for C in (3, 16):
        g = torch.Generator(device=dev).manual_seed(100 + C)
        with torch.no_grad():
            values = r.interpolate(ids, bary, torch.rand((verts.shape[0], C), device=dev, generator=g), faces)
        opacity = torch.rand(faces.shape[0], device=dev, generator=g) * 0.9 + 0.05
        for per_face in (False, True):
            out.append(case(r, ids, values, opacity, per_face, reps, warmup))
        del values
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cfg4", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("composite_time.py needs a GPU")
    dev = "cuda"
    out = dict(tool="composite_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
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
