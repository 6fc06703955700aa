#!/usr/bin/env python3
"""Randomised sweep of LayeredRenderer.generate on the HIP path against the CPU oracle: random lattice sizes, jitter,
face-existence density and values (0 / 1, or any non-zero value for "exists"), deleted tets, image sizes, cameras and layer
counts; both tet walks (packed per-tet records -- the default -- and the reference's access pattern under
DM2_FLAG_LEGACY_KERNELS).  Face ids and counts must match exactly.
`python tests/fuzz_layers.py [seconds] [seed]` runs it for as long as asked (needs a GPU).  Drawing a case (``draw``) and
building its scene (``scene``) need no GPU and are importable: tests/test_gpu_generate.py runs the fixed set ``GATE`` of them
as a parametrised test, so a seeded part of this sweep is part of the gate (with the structured scenes of
tests/tet_scenes.py, next to test_gpu_parity.py::test_layers_exact and test_gpu_scale.py::test_cfg3_layered_renderer_full_size);
the open-ended run stays a development tool."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

# what a case is drawn from
JITTERS = (0.0, 0.1, 0.2, 0.35)
EXISTENCE = (0.05, 0.3, 0.7, 1.0)
CAMS = (1, 2)
LAYERS = (1, 2, 3, 4, 5, 6)
HOLES = (0.0, 0.0, 0.1, 0.3)                 # share of tets deleted (half the cases keep them all)
EXISTENCE_VALUES = ("binary", "odd")         # flags of 0 / 1, or of 0, 1, 2, -1, INT_MIN


def draw(seed, idx):
    """The parameters of case ``idx`` of sweep ``seed`` (no GPU, nothing built)."""
    rng = np.random.default_rng([seed, idx])
    W, H = int(rng.integers(8, 200)), int(rng.integers(8, 140))
    n = int(rng.integers(1, 8))
    L = int(rng.integers(LAYERS[0], LAYERS[-1] + 1))
    cams = int(rng.integers(CAMS[0], CAMS[-1] + 1))
    jitter = float(rng.choice(JITTERS))
    ex = float(rng.choice(EXISTENCE))
    bidx = [int(b) for b in rng.integers(0, cams, size=int(rng.integers(1, 3)))]
    holes = float(rng.choice(HOLES))
    values = str(rng.choice(EXISTENCE_VALUES))
    return dict(seed=seed, idx=idx, W=W, H=H, n=n, L=L, cams=cams, jitter=jitter, existence=ex, bidx=bidx, holes=holes, values=values)


def scene(p):
    """The scenes.TetScene of the drawn parameters ``p`` (CPU tensors)."""
    import tet_scenes
    from dmesh2_renderer_amd import scenes
    sc = scenes.tet_lattice(p["W"], p["H"], p["n"], seed=scenes.SEED_BASE + 5000 + p["idx"] + 7919 * p["seed"], jitter=p["jitter"],
                            existence_p=p["existence"], num_cams=p["cams"])
    rng = np.random.default_rng([p["seed"], p["idx"], 1])
    if p["holes"] > 0:
        sc = tet_scenes.delete_tets(sc, rng.uniform(size=sc.tets.shape[0]) < p["holes"])
    if p["values"] == "odd":
        ex = sc.faces_existence.numpy()
        odd = np.asarray([v for v in tet_scenes.ODD_VALUES if v != 0], np.int64)[rng.integers(0, len(tet_scenes.ODD_VALUES) - 1, len(ex))]
        sc = tet_scenes.with_existence(sc, np.where(ex != 0, odd, 0).astype(np.int32))
    return sc


def run_case(p):
    """Case ``p`` on the GPU, both walks, against the oracle -> (ok, share of pixels with a layer)."""
    import dmesh2_renderer_amd as dm2
    from dmesh2_renderer_amd import _C
    from oracle import cpu as orc
    sc = scene(p)
    W, H, L, bidx = p["W"], p["H"], p["L"], p["bidx"]
    scd = sc.to("cuda")
    lr = dm2.LayeredRenderer(scd.mv, scd.proj, W, H, "cuda", fused_prep=False)
    ndc, img = lr.compute_verts_ndc_image(scd.verts, scd.mv[bidx], scd.proj[bidx])
    ro, rd = lr.ray_o[bidx], lr.ray_d[bidx]
    rl, rc = orc.generate_render_layers_cuda(W, H, sc.verts.numpy(), sc.faces.numpy(), sc.tets.numpy(), sc.face_tets.numpy(),
                                             sc.tet_faces.numpy(), sc.faces_existence.numpy(), ndc.cpu().numpy(), img.cpu().numpy(),
                                             ro.cpu().numpy(), rd.cpu().numpy(), L)[:2]
    ok = True
    for legacy in (0, _C.DM2_FLAG_LEGACY_KERNELS):
        old = _C.set_flags(legacy)
        try:
            layers, cnt = lr.generate(bidx, scd.verts, scd.faces, scd.tets, scd.face_tets, scd.tet_faces, scd.faces_existence, L)
        finally:
            _C.set_flags(old)
        ok = ok and np.array_equal(layers.cpu().numpy(), rl) and np.array_equal(cnt.cpu().numpy(), rc)
    return ok, float((rc > 0).mean())


def one_case(seed, idx):
    p = draw(seed, idx)
    ok, hit = run_case(p)
    return ok, dict(p, hit=hit)


# ---- the part of the sweep that every suite run executes -------------------------------------------------------------------
GATE_SEED, GATE_FIRST = 0, 24                # cases 0 .. 23 of sweep 0 ...


def _first(seed, want, start=0, stop=100000):
    for idx in range(start, stop):
        if want(draw(seed, idx)):
            return idx
    raise LookupError("no such case drawn")


def gate():
    """[(seed, idx)]: the first GATE_FIRST cases of sweep GATE_SEED, plus the first case drawn with jitter 0.0 and existence 1.0
    (an exact lattice, every face listed: rays in face planes) and the first with that and deleted tets."""
    ids = list(range(GATE_FIRST))
    for want in (lambda p: p["jitter"] == 0.0 and p["existence"] == 1.0 and p["holes"] == 0.0 and p["n"] >= 2,
                 lambda p: p["jitter"] == 0.0 and p["existence"] == 1.0 and p["holes"] > 0.0 and p["n"] >= 2):
        i = _first(GATE_SEED, want)
        if i not in ids:
            ids.append(i)
    return [(GATE_SEED, i) for i in ids]


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    t0, n, bad = time.time(), 0, 0
    while time.time() - t0 < budget:
        ok, desc = one_case(seed, n)
        n += 1
        if not ok:
            bad += 1
            print("MISMATCH", desc, flush=True)
        if n % 100 == 0:
            print(f"... {n} cases, {time.time() - t0:.0f} s", flush=True)
    print(f"{n} cases in {time.time() - t0:.0f} s, mismatches: {bad}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
