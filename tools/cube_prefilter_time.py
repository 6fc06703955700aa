"""Time Renderer.cube_prefilter (dm2_cube_prefilter / dm2_cube_prefilter_backward), forward under
no_grad and forward + backward (the cube requiring grad), with ``norm`` supplied and with ``norm=None`` (built in the call), at
N = 64, 256, 512 with ``max_mip_level`` chosen so that the last level has faces of 16^2, C = 3.  One JSON line.

    python tools/cube_prefilter_time.py [--reps 10] [--warmup 2] [--faces 64 256 512]

Baseline ``dense``: the route without the op, a torch matmul per level with that level's operator K(o,s) Om_s materialised once
outside the timed region ((6 n^2)^2 floats: 151 MB at 32^2 faces, 2.4 GB at 64^2), the box chain and the division by the norm as
in the op, with autograd.  It covers the levels with faces up to 32^2 only (``dense_levels``): at N = 64 that is the whole chain
and the two columns compare; above, the dense route does a part of the work, and the op's time on those same levels alone is
not separated.

Operation model, ``pairs``: the op evaluates the lobe for every (output, source) pair of the tiles that can hold a member:
all (6 n^2)^2 pairs of a level where the whole hemisphere takes part (r >= 0.298) up to the tiles a ball test drops (about the
far hemisphere's), fewer where the cut bites.  ``all_pairs`` is the sum of (6 n^2)^2 over the levels; a pair costs about 30 fp32
operations (one IEEE division among them) plus 2 per channel, and reads one 16-byte row plus the channel chunk from LDS as a
broadcast.  The candidates alternate step by step in one process on the same inputs; device events round each step; median
and the 10th / 90th percentile over --reps after --warmup.
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
from texture_cube_time import alternate  # noqa: E402

DENSE_MAX_FACE = 32
# face -> ((axis of sc, sign), (axis of tc, sign)): the lookup's table
FACE_ST = (((2, -1), (1, -1)), ((2, 1), (1, -1)), ((0, 1), (2, 1)), ((0, 1), (2, -1)), ((0, 1), (1, -1)), ((0, -1), (1, -1)))


def dense_operator(n, r, dev):
    """K(o,s) Om_s of one level as a (6 n^2, 6 n^2) float32 matrix, in torch (the baseline's: rounded as torch rounds it)."""
    c = (2 * (torch.arange(n, device=dev, dtype=torch.float32) + 0.5)) / n - 1
    tc, sc = torch.meshgrid(c, c, indexing="ij")
    q = 1 + sc * sc + tc * tc
    rq = q.sqrt()
    d = torch.zeros((6, n, n, 3), device=dev)
    for face, ((a, sa), (b, sb)) in enumerate(FACE_ST):
        d[face, :, :, face // 2] = -1.0 if face % 2 else 1.0
        d[face, :, :, a], d[face, :, :, b] = sa * sc, sb * tc
    d = (d / rq[None, :, :, None]).reshape(-1, 3)
    om = (1 / (q * rq)).expand(6, n, n).reshape(-1)
    m = torch.cdist(d, d).square()
    a2 = r ** 4
    cos = 1 - 0.5 * m
    e = a2 + (1 - a2) * (0.25 * m)
    K = torch.where((cos > 0) & (e <= 64 * a2), (a2 / e).square() * cos, torch.zeros_like(m))
    return K * om[None, :]


def case(r, N, C, reps, warmup):
    dev = torch.device("cuda")
    mx = max(N.bit_length() - 5, 0)                                      # the last level: 16^2
    nlev, levels, T = _C.mip_layout(N, N, mx)
    g = torch.Generator(device=dev).manual_seed(N)
    tex = torch.randn((6, N, N, C), device=dev, generator=g).requires_grad_(True)
    gout = torch.randn((6, T, C), device=dev, generator=g)
    norm = dm2.Renderer.cube_prefilter_norm(N, mx, device=dev)
    dense_levels = [(k, n, off) for k, (n, _, off) in enumerate(levels) if k >= 1 and n <= DENSE_MAX_FACE]
    ops = {k: dense_operator(n, k / (nlev - 1), dev) for k, n, _ in dense_levels}

    def dense():
        chain = r.texture_mipmaps(tex, mx)
        parts = []
        for k, n, off in dense_levels:
            x = chain[:, off:off + n * n].reshape(6 * n * n, C)
            parts.append(((ops[k] @ x).reshape(6, n * n, C) / norm[:, off:off + n * n, None]))
        return torch.cat(parts, 1)

    lo = dense_levels[0][2]
    with torch.no_grad():
        agree = float((r.cube_prefilter(tex, mx, norm=norm)[:, lo:] - dense()).abs().max())
    names = dict(op=lambda: r.cube_prefilter(tex, mx, norm=norm), op_norm_none=lambda: r.cube_prefilter(tex, mx),
                 dense=dense)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def fwd_bwd(fn, gr):
        def run():
            tex.grad = None
            fn().backward(gr)
        return run

    res = dict(N=N, C=C, max_mip_level=mx, nlev=nlev, faces=[n for n, _, _ in levels[1:]],
               roughness=[round(k / (nlev - 1), 4) for k in range(1, nlev)], dense_levels=[n for _, n, _ in dense_levels],
               all_pairs=sum((6 * n * n) ** 2 for n, _, _ in levels[1:]), max_abs_op_minus_dense=agree,
               fwd=alternate({k: fwd(v) for k, v in names.items()}, reps, warmup),
               fwd_bwd=alternate({k: fwd_bwd(v, gout[:, lo:] if k == "dense" else gout) for k, v in names.items()}, reps, warmup))
    res["fwd"]["op_all_pairs_per_ns"] = round(res["all_pairs"] / (res["fwd"]["op"]["ms"] * 1e6), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--faces", type=int, nargs="+", default=[64, 256, 512])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cube_prefilter_time.py needs a GPU")
    mv, proj = scenes.camera(32, 16)
    r = dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")
    out = dict(tool="cube_prefilter_time", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               cases=[case(r, N, 3, a.reps, a.warmup) for N in a.faces])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
