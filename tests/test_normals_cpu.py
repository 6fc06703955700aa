"""Renderer.vertex_adjacency and the restatement of Renderer.vertex_normals (tests/normals_ref.py), without a GPU: the index
against a plain loop, the forward on meshes whose normals are known exactly, float32 against float64 within a bound derived
from the list length and the cancellation, and grads64 against float64 central differences."""
import numpy as np
import pytest
import torch

import normals_ref as nref

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

EPS32 = float(np.finfo(np.float32).eps)


def _random_faces(rng, F, P, bad_every=5):
    faces = rng.integers(0, max(P, 1), (F, 3)).astype(np.int64)
    faces[::bad_every, rng.integers(0, 3)] = P + 2                         # out of range above
    faces[2::bad_every * 2, 0] = -1                                        # and below
    return faces


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.int16])
def test_adjacency_equals_a_plain_loop(dtype):
    rng = np.random.default_rng(5)
    P, F = 37, 211
    faces = _random_faces(rng, F, P)
    off, cor = dm2.Renderer.vertex_adjacency(torch.from_numpy(faces).to(dtype), P)
    assert off.dtype == torch.int32 and cor.dtype == torch.int32 and tuple(off.shape) == (P + 1,) and tuple(cor.shape) == (3 * F,)
    woff, wcor = nref.adjacency(faces, P)
    assert np.array_equal(off.numpy(), woff) and np.array_equal(cor.numpy(), wcor)
    # every valid corner exactly once, under its vertex, ascending; the invalid faces' corners behind offsets[P]
    valid = ((faces >= 0) & (faces < P)).all(1)
    off, cor = off.numpy(), cor.numpy()
    assert off[0] == 0 and off[P] == 3 * valid.sum() and (np.diff(off) >= 0).all()
    assert sorted(cor.tolist()) == list(range(3 * F))
    for p in range(P):
        mine = cor[off[p]:off[p + 1]]
        assert (np.diff(mine) > 0).all() and (faces.reshape(-1)[mine] == p).all() and valid[mine // 3].all()
    assert not valid[cor[off[P]:] // 3].any() and (~valid).any()
    assert dm2.LayeredRenderer.vertex_adjacency is dm2.Renderer.vertex_adjacency


def test_adjacency_of_nothing():
    off, cor = dm2.Renderer.vertex_adjacency(torch.zeros((0, 3), dtype=torch.int32), 4)
    assert off.tolist() == [0] * 5 and cor.numel() == 0 and cor.dtype == torch.int32
    off, cor = dm2.Renderer.vertex_adjacency(torch.tensor([[0, 1, 2], [0, 0, 0]]), 0)        # P = 0: every face is invalid
    assert off.tolist() == [0] and cor.tolist() == list(range(6))
    off, cor = dm2.Renderer.vertex_adjacency(torch.zeros((0, 3), dtype=torch.int64), 0)
    assert off.tolist() == [0] and cor.numel() == 0
    for a, b in ((nref.adjacency(np.zeros((0, 3), int), 4), ([0] * 5, [])), (nref.adjacency(np.zeros((0, 3), int), 0), ([0], []))):
        assert a[0].tolist() == b[0] and a[1].tolist() == b[1]
    with pytest.raises(ValueError, match="faces"):
        dm2.Renderer.vertex_adjacency(torch.zeros((3, 4), dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="integer"):
        dm2.Renderer.vertex_adjacency(torch.zeros((3, 3)), 4)
    with pytest.raises(ValueError, match="num_verts"):
        dm2.Renderer.vertex_adjacency(torch.zeros((3, 3), dtype=torch.int32), -1)


def test_octahedron_gives_the_axes_exactly():
    verts, faces = nref.octahedron()
    off, cor = nref.adjacency(faces, 6)
    assert (np.diff(off) == 4).all()
    n = nref.normals32(verts, faces, off, cor)
    assert np.array_equal(n, verts) and n.dtype == np.float32           # outward, unit, exact: all sums are integers
    s = nref.normals32(verts, faces, off, cor, normalize=False)
    assert np.array_equal(s, 4 * verts)


def test_soup_gives_each_face_its_own_normal():
    rng = np.random.default_rng(9)
    F = 50
    verts = rng.uniform(-1, 1, (3 * F, 3)).astype(np.float32)
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    off, cor = nref.adjacency(faces, 3 * F)
    e1, e2 = verts[1::3] - verts[0::3], verts[2::3] - verts[0::3]
    N = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    n = nref.normals32(verts, faces, off, cor)
    assert np.abs(n - np.repeat(N, 3, 0)).max() <= 8 * EPS32
    assert np.array_equal(n[0::3], n[1::3]) and np.array_equal(n[0::3], n[2::3])


@pytest.mark.parametrize("mesh", ["fan300", "random", "edge"])
def test_float32_against_float64_within_the_derived_bound(mesh):
    """s32 differs from the float64 sum by at most (k + 6) u s_abs per component, u = eps32 / 2, k the list length: two roundings in
    the edges, one per product, one in the difference, k in the running sum.  Normalised, the direction moves by at most twice that
    over |s| (the cancellation ratio sum|N| / |s| sits in s_abs / |s|) plus the roundings of sqrt and division."""
    if mesh == "fan300":
        verts, faces = nref.fan(300)
    elif mesh == "edge":
        verts, faces = nref.edge_mesh()
    else:
        rng = np.random.default_rng(2)
        verts = rng.uniform(-1, 1, (60, 3)).astype(np.float32)
        faces = _random_faces(rng, 400, 60, bad_every=9)
    P = verts.shape[0]
    off, cor = nref.adjacency(faces, P)
    k = np.diff(off).astype(np.float64)[:, None]
    u = EPS32 / 2
    _, s64, sa = nref.normals64(verts, faces)
    s32 = nref.normals32(verts, faces, off, cor, normalize=False).astype(np.float64)
    bound_s = (k + 6) * u * sa
    assert (np.abs(s32 - s64) <= bound_s).all()
    n64 = nref.normals64(verts, faces)[0]
    n32 = nref.normals32(verts, faces, off, cor).astype(np.float64)
    ln = np.linalg.norm(s64, axis=1, keepdims=True)
    live = ln[:, 0] > 0
    bound_n = 2 * np.linalg.norm(bound_s, axis=1, keepdims=True) / np.where(live[:, None], ln, 1.0) + 4 * EPS32
    assert (np.abs(n32 - n64)[live] <= bound_n[live]).all()
    assert not n32[~live].any() and not n64[~live].any()
    if mesh == "edge":
        assert not live[[8, 12, 13]].any() and live.sum() == P - 3
    assert np.abs(np.linalg.norm(n32[live], axis=1) - 1).max() <= 4 * EPS32


@pytest.mark.parametrize("mesh", ["closed", "fan300", "edge"])
@pytest.mark.parametrize("normalize", [True, False])
def test_grads64_against_central_differences(mesh, normalize):
    if mesh == "closed":
        verts, faces = nref.octahedron()
        verts = verts + np.random.default_rng(1).uniform(-0.2, 0.2, verts.shape).astype(np.float32)
    elif mesh == "fan300":
        verts, faces = nref.fan(300)
    else:
        verts, faces = nref.edge_mesh()
    g = np.random.default_rng(4).standard_normal(verts.shape)
    got, sabs = nref.grads64(verts, faces, g, normalize)
    want = nref.central_differences(verts, faces, g, normalize)
    assert np.abs(want).max() > 0
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert (np.abs(got) <= sabs * (1 + 1e-12)).all()                     # the abs-evaluated sum dominates the sum
    if mesh == "edge":
        assert not got[[12, 13]].any() and not sabs[[12, 13]].any()       # isolated: nothing contributes
        if normalize:
            only8 = np.zeros_like(g)
            only8[8] = g[8]
            assert not nref.grads64(verts, faces, only8, True)[0].any()   # the cancelled vertex sends its gradient nowhere


def test_surface():
    for name in ("VertexNormalsFunction", "ShadingVectorsFunction"):
        assert name in dm2.__all__ and issubclass(getattr(dm2, name), torch.autograd.Function)
    for name in ("dm2_vertex_normals", "dm2_vertex_normals_backward", "dm2_vertex_normals_scratch_bytes"):
        assert name in _C.EXPORTS
    for cls in (dm2.Renderer, dm2.LayeredRenderer):
        assert callable(cls.vertex_normals) and callable(cls.vertex_adjacency) and callable(cls.shading_vectors)
    verts, faces = nref.octahedron()
    off, cor = dm2.Renderer.vertex_adjacency(torch.from_numpy(faces), 6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.vertex_normals_cuda(torch.from_numpy(verts), torch.from_numpy(faces), off, cor)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dm2.Renderer.vertex_normals(None, torch.from_numpy(verts), torch.from_numpy(faces))
