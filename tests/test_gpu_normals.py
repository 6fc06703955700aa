"""Renderer.vertex_adjacency / Renderer.vertex_normals on the GPU against tests/normals_ref.py: the forward bit for bit, the
gradient per element within  |g - g64| <= 1e-5 max|g64| + 8 eps32 sum|terms|  (util.summation_bound) with exact zeros where
nothing contributes, two backward calls bit-equal (no atomics), no kernel where no gradient is asked for, unaligned and
non-contiguous inputs, and the argument checks down to the C ABI."""
import functools

import numpy as np
import pytest
import torch

import normals_ref as nref
import rasterize_ref as rref
from util import patched_C, scenes, summation_bound

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
MESHES = ("octahedron", "soup", "lattice", "degenerate", "no_faces", "tet_lattice", "fan300", "fan2000", "edge", "random")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(verts, faces, offsets, corners) float32 / int32 numpy; the index by the plain loop of the restatement."""
    if name == "octahedron":
        verts, faces = nref.octahedron()
    elif name in rref.SCENES:
        s = rref.scene(name)
        verts, faces = s["verts"], s["faces"]
    elif name == "tet_lattice":
        ts = scenes.tet_lattice(32, 32, 5, seed=scenes.SEED_BASE + 90)
        verts, faces = ts.verts.numpy(), ts.faces.numpy()
    elif name.startswith("fan"):
        verts, faces = nref.fan(int(name[3:]))                             # 300: the hub's list crosses a wave; 2000: a block
    elif name == "edge":
        verts, faces = nref.edge_mesh()
    else:                                                                  # P = 2 blocks + 1, invalid faces scattered
        rng = np.random.default_rng(12)
        P = 513
        verts = rng.uniform(-1, 1, (P, 3)).astype(f32)
        faces = rng.integers(0, P, (1500, 3)).astype(np.int32)
        faces[::17, 1] = P
        faces[5::29, 2] = -3
    verts, faces = np.ascontiguousarray(verts, f32), np.ascontiguousarray(faces, np.int32)
    assert name != "random" or verts.shape[0] % 256 == 1
    return (verts, faces) + nref.adjacency(faces, verts.shape[0])


def _renderer():
    mv, proj = scenes.camera(16, 16)
    return dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 16, 16, "cuda")


@pytest.mark.parametrize("name", MESHES)
def test_adjacency_on_the_gpu_equals_the_cpu(name):
    verts, faces, woff, wcor = _mesh(name)
    P = verts.shape[0]
    for dtype in (torch.int32, torch.int64):
        off, cor = dm2.Renderer.vertex_adjacency(_cu(faces).to(dtype), P)
        assert off.is_cuda and off.dtype == torch.int32 and cor.dtype == torch.int32
        assert np.array_equal(off.cpu().numpy(), woff) and np.array_equal(cor.cpu().numpy(), wcor)
    coff, ccor = dm2.Renderer.vertex_adjacency(torch.from_numpy(faces), P)
    assert np.array_equal(coff.numpy(), woff) and np.array_equal(ccor.numpy(), wcor)


@pytest.mark.parametrize("name", MESHES)
def test_forward_bit_equal_to_the_restatement(name):
    verts, faces, off, cor = _mesh(name)
    r = _renderer()
    for normalize in (True, False):
        want = nref.normals32(verts, faces, off, cor, normalize)
        built = r.vertex_normals(_cu(verts), _cu(faces), normalize=normalize)
        passed = r.vertex_normals(_cu(verts), _cu(faces), adjacency=(_cu(off), _cu(cor)), normalize=normalize)
        torch.cuda.synchronize()
        assert built.dtype == torch.float32 and tuple(built.shape) == verts.shape
        assert np.array_equal(_bits(built.cpu().numpy()), _bits(want)), (name, normalize)
        assert torch.equal(built, passed)
    if name == "octahedron":
        assert np.array_equal(want, 4 * verts)
    if name == "no_faces":
        assert not want.any()
    if name == "fan2000":
        assert off[1] - off[0] == 2000
    if name == "edge":
        huge = (verts * f32(1e25)).astype(f32)                             # every face normal overflows: zeros, not NaN
        got = r.vertex_normals(_cu(huge), _cu(faces)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(nref.normals32(huge, faces, off, cor))) and not got.any()


def _grad(r, verts, faces, g, normalize, adjacency=None):
    v = _cu(verts).requires_grad_(True)
    n = r.vertex_normals(v, _cu(faces), adjacency=adjacency, normalize=normalize)
    n.backward(_cu(g))
    torch.cuda.synchronize()
    return v.grad


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("normalize", [True, False])
def test_gradient_within_the_criterion_and_reproducible(name, normalize):
    verts, faces, off, cor = _mesh(name)
    P = verts.shape[0]
    r = _renderer()
    g = np.random.default_rng(21).standard_normal((P, 3)).astype(f32)
    got_t = _grad(r, verts, faces, g, normalize)
    again = _grad(r, verts, faces, g, normalize, adjacency=(_cu(off), _cu(cor)))
    assert torch.equal(got_t, again)                                       # no atomics: the same bits
    assert np.array_equal(_bits(got_t.cpu().numpy()), _bits(again.cpu().numpy()))
    got = got_t.cpu().numpy().astype(np.float64)
    want, sabs = nref.grads64(verts, faces, g, normalize)
    assert np.isfinite(got).all()
    assert not got[sabs == 0].any()                                        # exact zeros where nothing contributes
    if name == "no_faces":
        assert not got.any() and not want.any()
        return
    gmax = np.abs(want).max()
    assert gmax > 0
    bound = summation_bound(gmax, sabs)
    ratio = (np.abs(got - want) / bound).max()
    print(f"vertex_normals {name} normalize={normalize}: worst error / bound {ratio:.3g}, rel L_inf {np.abs(got - want).max() / gmax:.3g}")
    assert (np.abs(got - want) <= bound).all(), (name, normalize, ratio)
    valid = ((faces >= 0) & (faces < P)).all(1)
    untouched = np.ones(P, bool)
    untouched[faces[valid].reshape(-1)] = False
    assert not got[untouched].any()
    if name == "edge" and normalize:
        only8 = np.zeros_like(g)
        only8[8] = g[8]
        assert not _grad(r, verts, faces, only8, True).any()               # the cancelled vertex sends its gradient nowhere


def test_no_gradient_asked_for_means_no_kernel():
    verts, faces, off, cor = _mesh("lattice")
    r = _renderer()
    calls = []
    real = _C.vertex_normals_backward_cuda

    def spy(*a):
        calls.append(1)
        return real(*a)

    with patched_C(vertex_normals_backward_cuda=spy):
        n = r.vertex_normals(_cu(verts), _cu(faces))
        assert not n.requires_grad
        v = _cu(verts).requires_grad_(True)
        n = r.vertex_normals(v, _cu(faces))
        assert n.requires_grad
        (v * 2.0).sum().backward()                                         # the normals are left out of the loss
        assert not calls
        with torch.no_grad():
            assert not r.vertex_normals(v, _cu(faces)).requires_grad
        out = dm2.VertexNormalsFunction.apply(v.detach(), _cu(faces), _cu(off), _cu(cor), True)
        assert not out.requires_grad and not calls
        (n * n).sum().backward()
        assert calls == [1]


def test_unaligned_and_non_contiguous_inputs():
    verts, faces, off, cor = _mesh("random")
    r = _renderer()
    g = np.random.default_rng(3).standard_normal(verts.shape).astype(f32)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = _cu(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    wide = torch.zeros((faces.shape[0], 5), dtype=torch.int32, device="cuda")
    wide[:, 1:4] = _cu(faces)
    fv = wide[:, 1:4]
    vt = torch.zeros((3, verts.shape[0]), device="cuda")
    vt[:] = _cu(verts).t()
    assert not fv.is_contiguous() and not vt.t().is_contiguous()
    want = nref.normals32(verts, faces, off, cor)
    base = _grad(r, verts, faces, g, True)
    for v_in in (shifted(verts), vt.t()):
        v = v_in.detach().requires_grad_(True)
        n = r.vertex_normals(v, fv)
        assert np.array_equal(_bits(n.detach().cpu().numpy()), _bits(want))
        n.backward(shifted(g))
        assert torch.equal(v.grad, base)


def test_argument_checks():
    verts, faces, off, cor = (_cu(x) for x in _mesh("edge"))
    r = _renderer()
    P, F = verts.shape[0], faces.shape[0]
    ok, lens = _C.vertex_normals_cuda(verts, faces, off, cor)
    assert tuple(ok.shape) == (P, 3) and tuple(lens.shape) == (P,)
    for args, name in (((verts[:, :2], faces, off, cor), "verts"), ((verts.double(), faces, off, cor), "verts"),
                       ((verts, faces[:, :2], off, cor), "faces"), ((verts, faces.long(), off, cor), "faces"),
                       ((verts, faces, off[:-1], cor), "offsets"), ((verts, faces, off.long(), cor), "offsets"),
                       ((verts, faces, off, cor[:-1]), "corners"), ((verts, faces, off, cor.float()), "corners")):
        with pytest.raises(RuntimeError, match=name):
            _C.vertex_normals_cuda(*args)
    with pytest.raises(RuntimeError, match="grad_normals"):
        _C.vertex_normals_backward_cuda(verts, faces, off, cor, True, ok, lens, ok[:, :2])
    with pytest.raises(RuntimeError, match="normals"):
        _C.vertex_normals_backward_cuda(verts, faces, off, cor, True, ok[:-1], lens, ok)
    with pytest.raises(RuntimeError, match="len"):
        _C.vertex_normals_backward_cuda(verts, faces, off, cor, True, ok, lens[:-1], ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.vertex_normals_cuda(verts.cpu(), faces.cpu(), off.cpu(), cor.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.vertex_normals(verts, faces.cpu())
    with pytest.raises(RuntimeError, match="offsets"):
        r.vertex_normals(verts, faces, adjacency=dm2.Renderer.vertex_adjacency(faces, P + 1))
    assert type(dm2.LayeredRenderer.vertex_normals) is type(dm2.Renderer.vertex_normals)
    # P = 0 and F = 0 launch nothing they should not
    e, _ = _C.vertex_normals_cuda(verts[:0], faces, *dm2.Renderer.vertex_adjacency(faces, 0))
    assert tuple(e.shape) == (0, 3)
    z, _ = _C.vertex_normals_cuda(verts, faces[:0], *dm2.Renderer.vertex_adjacency(faces[:0], P))
    assert not z.any()
    # the C ABI refuses what the shim would never send
    lib = _C.load_library()
    p = _C._ptr
    need = lib.dm2_vertex_normals_scratch_bytes(P, F, 0)
    assert need == 16 * F and lib.dm2_vertex_normals_scratch_bytes(P, F, 1) == 16 * (P + 3 * F)
    scratch = torch.empty(16 * (P + 3 * F) + 16, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(ok)
    base = (P, F, 1, p(verts), p(faces), p(off), p(cor))
    assert lib.dm2_vertex_normals(*base, p(scratch), need, p(out), p(lens), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ok)
    assert lib.dm2_vertex_normals(*base, p(scratch), need - 1, p(out), p(lens), None) == 1
    assert b"scratch" in lib.dm2_last_error()
    assert lib.dm2_vertex_normals(*base, None, need, p(out), p(lens), None) == 1
    assert lib.dm2_vertex_normals(*base, p(scratch[4:]), need, p(out), p(lens), None) == 1
    assert lib.dm2_vertex_normals(*base, p(scratch), need, None, p(lens), None) == 1
    assert lib.dm2_vertex_normals(-1, F, 1, *base[3:], p(scratch), need, p(out), p(lens), None) == 1
    assert lib.dm2_vertex_normals(P, 2 ** 30, 1, *base[3:], p(scratch), need, p(out), p(lens), None) == 1
    assert lib.dm2_vertex_normals(P, F, 1, None, *base[4:], p(scratch), need, p(out), p(lens), None) == 1
    assert lib.dm2_vertex_normals_backward(*base, p(ok), p(lens), p(ok), p(scratch), need, p(out), None) == 1      # the forward's size
    assert lib.dm2_vertex_normals_backward(*base, None, p(lens), p(ok), p(scratch), 16 * (P + 3 * F), p(out), None) == 1
    torch.cuda.synchronize()
