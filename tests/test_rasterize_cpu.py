"""Renderer.rasterize / dm2_rasterize_run without a GPU: the contract's restatement (tests/rasterize_ref.py) against the
CPU oracle's ray/triangle test and its tet walk, the kernel's early exit against the contract on every scene the GPU tests
use, and the module's refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import layer_composite_ref as lref
import rasterize_ref as ref
from util import ROOT  # noqa: F401  (puts the repository on sys.path)

from dmesh2_renderer_amd import scenes


def test_ray_tri32_bit_equal_to_oracle_near_edges():
    """ray_tri32 gives the oracle's Moeller-Trumbore bit for bit on random (ray, triangle) pairs, a third of them aimed at a
    point of an edge or a corner (u, v or 1 - u - v within a few ulps of 0), where the hit test's >= 0 decides."""
    from oracle import cpu as orc
    rng = np.random.RandomState(11)
    n = 3000
    p = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
    ro = rng.uniform(-1, 1, (n, 3)).astype(np.float32) + np.float32(3) * np.array([0, 0, 1], np.float32)
    target = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    k = np.arange(n) % 3 == 0
    a, b = rng.randint(0, 3, n), rng.uniform(0, 1, n)
    edge = (p[np.arange(n), a] * (1 - b)[:, None] + p[np.arange(n), (a + 1) % 3] * b[:, None]).astype(np.float32)
    edge[::9] = p[::9, 0]                                                         # exact corners
    target[k] = edge[k]
    rd = (target - ro).astype(np.float32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True).astype(np.float32)
    ok, t, u, v = lref.ray_tri32(ro, rd, p[:, 0], p[:, 1], p[:, 2])
    near = 0
    for i in range(n):
        ok_o, tuv, _ = orc.ray_tri(ro[i], rd[i], p[i].reshape(-1), np.float32)
        assert ok_o == bool(ok[i]), i
        if not ok_o:
            continue
        got = np.array([t[i], u[i], v[i]], np.float32)
        assert np.array_equal(got.view(np.uint32), tuv.astype(np.float32).view(np.uint32)), (i, got, tuv)
        near += int(min(abs(u[i]), abs(v[i]), abs(np.float32(1) - u[i] - v[i])) < 1e-6)
    assert near > 300


@pytest.mark.parametrize("name", ref.SCENES)
def test_early_exit_changes_no_list(name):
    """The kernel's depth stop (a face whose min depth lies beyond the largest max depth of a full set of held hits cannot
    come nearer) leaves every list of every scene the GPU tests use as the contract defines it, for every L they use."""
    s = ref.scene(name)
    stopped = 0
    for fe in (None, s["fe"]):
        x = ref.intersect(s["W"], s["H"], s["verts"], s["faces"], fe, s["verts_ndc"], s["verts_image"], s["ray_o"], s["ray_d"])
        for L in (1, 3, 8, 16, 17, 40):
            want = ref.select(x, L)
            got = ref.select(x, L, early_exit=True)
            for k in ("layers", "cnt", "bary", "t"):
                assert np.array_equal(got[k], want[k]), (name, fe is None, L, k)
            stopped += int((want["cnt"] == L).sum())
    if name != "no_faces":
        assert stopped > 0                                          # (full lists: the stop had a chance to act)


def test_restatement_on_hand_cases():
    """One frame-filling triangle in front of another: ids in depth order, t the distance along the ray, bary reproduces the
    hit point; an existence flag of 0 removes a face; empty slots hold -1."""
    W = H = 16
    mv, proj = scenes.camera(W, H)
    from oracle import cpu as orc
    verts = np.array([[-4, -4, 0], [8, -4, 0], [-4, 8, 0], [-4, -4, 1], [8, -4, 1], [-4, 8, 1]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)                            # the far face first in id order
    prep = orc.prepare_faces(verts, faces, mv[None], proj[None], W, H)
    ro, rd = orc.analytic_rays(mv[None], proj[None], W, H)
    r = ref.rasterize32(W, H, verts, faces, None, prep["verts_ndc"], prep["verts_image"], ro, rd, 3)
    assert np.all(r["cnt"] == 2)
    near, far = r["layers"][..., 0], r["layers"][..., 1]
    assert np.all(near == 1) and np.all(far == 0)
    assert np.all(r["layers"][..., 2] == -1) and np.all(r["bary"][..., 2, :] == -1) and np.all(r["t"][..., 2] == -1)
    hit = ro[..., None, :] + r["t"][..., :2, None] * rd[..., None, :]
    corners = verts[faces[r["layers"][..., :2]]]                                   # (B,H,W,2,3,3)
    interp = (r["bary"][..., :2, :, None] * corners).sum(-2)
    assert np.abs(hit - interp).max() < 1e-5
    assert np.allclose(hit[..., 0, 2], 1.0, atol=1e-5) and np.allclose(hit[..., 1, 2], 0.0, atol=1e-5)
    fe = np.array([1, 0], np.int32)
    r2 = ref.rasterize32(W, H, verts, faces, fe, prep["verts_ndc"], prep["verts_image"], ro, rd, 3)
    assert np.array_equal(r2["layers"][..., 0], far) and np.all(r2["cnt"] == 1)


@pytest.mark.parametrize("n,seed", [(4, 70), (6, 71)])
def test_generate_layers_are_a_prefix_of_the_restatement(n, seed):
    """On tet lattices inside the NDC depth range the oracle's tet walk lists, at every pixel, a prefix of the restatement's
    list -- except where two listed faces lie within 1e-6 t of each other along the ray (a ray through a shared edge or
    vertex: the walk stops there, or the order of the two is a coin toss)."""
    from oracle import cpu as orc
    W, H, L, views = 96, 72, 8, [1, 0]
    ts = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + seed, num_cams=2)
    mv, proj = ts.mv[views], ts.proj[views]
    prep = orc.prepare_faces(ts.verts, ts.faces, mv, proj, W, H)
    ndc, img = prep["verts_ndc"], prep["verts_image"]
    assert np.all(np.abs(ndc[..., 2]) < 1)                                          # inside the depth range: nothing culled
    ro, rd = orc.analytic_rays(mv, proj, W, H)
    fe = ts.faces_existence.numpy()
    gl, gc = orc.generate_render_layers_cuda(W, H, ts.verts, ts.faces, ts.tets, ts.face_tets, ts.tet_faces, fe, ndc, img, ro, rd, L)
    r = ref.rasterize32(W, H, ts.verts, ts.faces, fe, ndc, img, ro, rd, L)
    bad = ref.prefix_violations(gl, gc, r)
    ties = ref.near_ties(r)
    excused = int((bad & ties).sum())
    print(f"tet_lattice(n={n}): {excused} of {bad.size} pixels excused (near-tie), generate lists {int(gc.sum())} faces, "
          f"rasterize {int(r['cnt'].sum())}")
    assert not (bad & ~ties).any(), np.argwhere(bad & ~ties)[:5]
    assert excused <= 0.001 * bad.size                                             # (measured: 0 on both lattices)
    assert gc.sum() > 0.3 * r["cnt"].sum()                                          # (the walk got somewhere)


def test_rasterize_refuses_cpu_tensors():
    import dmesh2_renderer_amd as dm2
    from dmesh2_renderer_amd import _C
    ts = scenes.tet_lattice(32, 24, 2, seed=scenes.SEED_BASE + 3)
    r = dm2.Renderer(ts.mv, ts.proj, 32, 24, "cpu", fused_prep=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.rasterize([0], ts.verts, ts.faces, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.rasterize([0], ts.verts, ts.faces, 4, faces_existence=ts.faces_existence)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 32, 24, "cpu", fused_prep=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lr.rasterize([0], ts.verts.requires_grad_(True), ts.faces, 2)
    layers = torch.zeros((1, 24, 32, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.rasterize_layers_backward_cuda(layers, ts.verts, ts.faces, r.ray_o, r.ray_d, None, torch.zeros((1, 24, 32, 2)))
