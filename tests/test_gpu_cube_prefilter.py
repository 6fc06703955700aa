"""Renderer.cube_prefilter / dm2_cube_prefilter on the GPU against the contract's restatement
(tests/cube_prefilter_ref.py): the whole operator from one one-hot call (exact zeros off the members, 4 * 2^-24 on them); dense
inputs, the transpose and the adjoint identity against the float64 sums under the derived bound (members + 4) 2^-24 sum |K Om x|;
determinism; the public op and its gradient; the path into texture(..., "cube", mip_level=...); refusals at the C ABI.

Worst error / bound ratios seen on MI355X are recorded in DESIGN.md section 8, "Prefiltered cube chains"."""
import ctypes

import numpy as np
import pytest
import torch

import cube_prefilter_ref as ref
import texture_cube_mip_ref as cmref
from util import scenes

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

# (N, C, B (None: one shared cube), max_mip_level)
DENSE = ((8, 3, None, None), (8, 5, 2, None), (12, 3, None, None), (48, 3, None, None), (16, 3, None, 2), (8, 1, None, None))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _prim(x, N, mx=None, transpose=False):
    f = _C.cube_prefilter_transpose_cuda if transpose else _C.cube_prefilter_cuda
    out = f(_cu(x), N, mx)
    torch.cuda.synchronize()
    return _np(out)


def _chain(seed, N, C, B, mx):
    rng = np.random.default_rng(seed)
    T = ref.layout(N, mx)[2]
    return rng.standard_normal(((B,) if B else ()) + (6, T, C), dtype=np.float32)


def _held(got, want, terms, members, what):
    """got within the derived bound of want, element by element -> the worst error / bound ratio."""
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all(), what
    b = ref.bound(terms, members)
    assert (b > 0).all(), what
    ratio = float((np.abs(got - want) / b).max())
    print(f"cube_prefilter {what}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)
    return ratio


def _renderer():
    mv, proj = scenes.camera(32, 16)
    return dm2.Renderer(mv[None].cuda(), proj[None].cuda(), 32, 16, "cuda")


def test_whole_operator_one_hot():
    """N = 16, levels 8, 4, 2, 1 (level 1: r = 0.25, the cut active): the identity over the 510 chain texels as 510 channels
    gives every K(o,s) Om_s in one call.  Zeros exactly where the restatement has none (another level, or no member); the
    others within 4 * 2^-24 relative (the roundings of K Om and of its product with x, with margin)."""
    N = 16
    nlev, levels, T = ref.layout(N)
    assert (nlev, 6 * T) == (5, 510)
    x = np.eye(6 * T, dtype=np.float32).reshape(6, T, 6 * T)
    got = _prim(x, N).reshape(6 * T, 6 * T).astype(np.float64)           # [o, s]
    want = np.zeros((6 * T, 6 * T))
    for k in range(1, nlev):
        n, _, off = levels[k]
        rows = (np.arange(6)[:, None] * T + off + np.arange(n * n)[None, :]).reshape(-1)      # level row -> chain row
        A, members = ref.operator(n, k, nlev)
        want[np.ix_(rows, rows)] = A
        if k == 1:
            assert members.min() < 6 * n * n // 2 - n                     # the cut is active: fewer than a hemisphere
    assert np.array_equal(got != 0, want != 0), int(((got != 0) != (want != 0)).sum())
    nz = want != 0
    rel = np.abs(got[nz] - want[nz]) / want[nz]
    print(f"cube_prefilter one-hot: {int(nz.sum())} entries, worst relative error = {rel.max() / ref.EPS:.3f} * 2^-24")
    assert rel.max() <= 4 * ref.EPS
    # the transpose of the same input: Om on the other side
    got_t = _prim(x, N, transpose=True).reshape(6 * T, 6 * T).astype(np.float64)       # [s, g's texel o]
    assert np.array_equal(got_t != 0, want.T != 0)
    assert (np.abs(got_t[nz.T] - want.T[nz.T]) / want.T[nz.T]).max() <= 4 * ref.EPS


@pytest.mark.parametrize("N,C,B,mx", DENSE)
def test_dense_forward_transpose_adjoint(N, C, B, mx):
    x, g = _chain(10 + N + C, N, C, B, mx), _chain(20 + N + C, N, C, B, mx)
    if B:
        assert np.abs(x[0] - x[1]).max() > 1                              # different cubes per view
    y = _prim(x, N, mx)
    y64, yterms, ymem = ref.primitive64(x, N, mx)
    _held(y, y64, yterms, ymem, ("forward", N, C, B, mx))
    xb = _prim(g, N, mx, transpose=True)
    xb64, xterms, xmem = ref.primitive64(g, N, mx, transpose=True)
    _held(xb, xb64, xterms, xmem, ("transpose", N, C, B, mx))
    # <primitive(x), g> = <x, transpose(g)>, in float64 from the GPU's outputs, within the two bounds
    lhs, rhs = (y.astype(np.float64) * g).sum(), (x.astype(np.float64) * xb).sum()
    slack = (np.abs(g) * ref.bound(yterms, ymem)).sum() + (np.abs(x) * ref.bound(xterms, xmem)).sum()
    assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)


@pytest.mark.parametrize("N,cases", ((128, ((1, True), (2, False))), (144, ((1, True),)), (132, ((1, False),))))
def test_many_tiles_sampled_rows(N, cases):
    """Faces of several tiles, on both sides of the size at which the kernel changes its block shape (64^2), rows sampled (the
    corners of every tile of two faces, where a skipped neighbour would show first, and random ones) against their float64
    sums under the same bound.  N = 128, full chain: level 1 has faces of 64^2 (4 x 4 tiles) at r = 1/7, where a texel's
    members span about a tile and most tiles are skipped, level 2 32^2 at r = 2/7, the cut barely active.  N = 144: level 1
    is 72^2 (4.5 tiles a side) at r = 0.25.  N = 132: level 1 is 66^2 at r = 0.5, the whole hemisphere."""
    C = 2
    nlev, levels, T = ref.layout(N)
    x = _chain(70 + N, N, C, None, None)
    y, xb = _prim(x, N), _prim(x, N, transpose=True)
    rng = np.random.default_rng(71)
    for k, narrow in cases:
        n, _, off = levels[k]
        edge = np.unique(np.concatenate([np.arange(0, n, 16), np.arange(15, n, 16), [n - 1]]))
        jj, ii = np.meshgrid(edge, edge, indexing="ij")
        rows = np.concatenate([(f * n * n + jj * n + ii).reshape(-1) for f in (0, 3)] + [rng.choice(6 * n * n, 64, replace=False)])
        K, member = ref.lobe(n, ref.roughness(k, nlev)[1], rows)
        assert (member.sum(1).max() < 0.3 * 6 * n * n) == narrow          # narrow: the skipping is at work
        _, om = ref.texels(n)
        xl = x[:, off:off + n * n].reshape(6 * n * n, C).astype(np.float64)
        K64, om64 = K.astype(np.float64), om.astype(np.float64)
        A = K64 * om64[None, :]
        mem = np.broadcast_to(member.sum(1)[:, None], (len(rows), C))
        _held(y[:, off:off + n * n].reshape(-1, C)[rows], A @ xl, A @ np.abs(xl), mem[..., 0], ("narrow forward", n))
        At = K64 * om64[rows][:, None]                                    # the transpose's rows: K is symmetric
        _held(xb[:, off:off + n * n].reshape(-1, C)[rows], At @ xl, At @ np.abs(xl), mem[..., 0], ("narrow transpose", n))


def test_determinism():
    for N, C, B, mx in ((48, 3, None, None), (16, 5, 2, None)):
        x = _chain(30 + N, N, C, B, mx)
        for transpose in (False, True):
            a, b = _prim(x, N, mx, transpose), _prim(x, N, mx, transpose)
            assert np.array_equal(_bits(a), _bits(b)), (N, transpose)


@pytest.mark.parametrize("N,C,B,mx", ((8, 3, None, None), (12, 2, 2, None), (16, 3, None, 2)))
def test_public_op_and_gradient(N, C, B, mx):
    r = _renderer()
    rng = np.random.default_rng(40 + N)
    tex = rng.standard_normal(((B,) if B else ()) + (6, N, N, C), dtype=np.float32)
    T = ref.layout(N, mx)[2]
    g = rng.standard_normal(tex.shape[:-3] + (T, C), dtype=np.float32)
    t = _cu(tex).requires_grad_(True)
    out = r.cube_prefilter(t, mx)
    want, tol = ref.prefilter64(tex, mx)
    assert out.shape == want.shape and out.dtype == torch.float32
    ratio = float((np.abs(_np(out) - want) / tol).max())
    print(f"cube_prefilter public op {(N, C, B, mx)}: worst error / tolerance = {ratio:.4f}")
    assert ratio <= 1.0
    out.backward(_cu(g))
    grad64, slack = ref.prefilter_backward64(tex.shape, mx, g)
    accept = 1e-5 * np.abs(grad64).max() + slack
    gr = float((np.abs(_np(t.grad) - grad64) / accept).max())
    print(f"cube_prefilter public gradient {(N, C, B, mx)}: worst error / acceptance = {gr:.4f}")
    assert t.grad.shape == t.shape and gr <= 1.0
    # norm supplied or built in the call: the same bits
    norm = dm2.Renderer.cube_prefilter_norm(N, mx, device="cuda")
    W, wb = ref.norm64(N, mx)
    assert norm.shape == (6, T) and (np.abs(_np(norm) - W) <= wb).all()
    assert np.array_equal(_bits(_np(r.cube_prefilter(_cu(tex), mx, norm=norm))), _bits(_np(out)))
    assert dm2.LayeredRenderer.cube_prefilter_norm(N, mx, device="cuda").equal(norm)


def test_constant_cube_and_empty_chain():
    r = _renderer()
    N, C = 16, 3
    c = np.array([0.75, -2.5, 1e-3], np.float32)
    tex = np.broadcast_to(c, (6, N, N, C)).copy()
    out = _np(r.cube_prefilter(_cu(tex)))
    _, tol = ref.prefilter64(tex)
    assert (np.abs(out - c.astype(np.float64)) <= tol).all()
    assert np.abs(out / c - 1).max() <= 1e-5
    odd = r.cube_prefilter(_cu(np.ones((2, 6, 5, 5, 2), np.float32)).requires_grad_(True))
    assert odd.shape == (2, 6, 0, 2)
    assert dm2.Renderer.cube_prefilter_norm(5, device="cuda").shape == (6, 0)


def test_end_to_end_into_the_cube_lookup():
    """texture(dirs, tex, rl, "linear-mipmap-linear", "cube", mip=cube_prefilter(tex), mip_level=level): tex.grad = the direct
    level-0 part + the chain's part (the restatement's dL/dmip) pushed through the filter's and the box chain's backwards."""
    r = _renderer()
    rng = np.random.default_rng(60)
    N, C, shape = 8, 3, (1, 8, 8, 2)
    nlev = ref.layout(N)[0]
    tex = rng.standard_normal((6, N, N, C), dtype=np.float32)
    dirs = rng.standard_normal(shape + (3,)).astype(np.float32)
    level = rng.uniform(0.05, nlev - 1.05, shape).astype(np.float32)
    rl = np.where(rng.uniform(size=shape) < 1 / 8, -1, 0).astype(np.int32)
    g = rng.standard_normal(shape + (C,), dtype=np.float32)
    t, lv = _cu(tex).requires_grad_(True), _cu(level).requires_grad_(True)
    mip = r.cube_prefilter(t)
    out = r.texture(_cu(dirs), t, _cu(rl), "linear-mipmap-linear", "cube", mip=mip, mip_level=lv)
    out.backward(_cu(g))
    wt, wm, _, wl, _ = cmref.grads64(dirs, level, tex, _np(mip), rl, None, g)
    chain_part, slack = ref.prefilter_backward64(tex.shape, None, wm)
    want = wt + chain_part
    assert np.abs(chain_part).max() > 0.1 * np.abs(wt).max() and np.abs(wt).max() > 0
    accept = 1e-5 * np.abs(want).max() + slack
    ratio = float((np.abs(_np(t.grad) - want) / accept).max())
    print(f"cube_prefilter end to end: worst error / acceptance = {ratio:.4f}")
    assert ratio <= 1.0
    assert lv.grad is not None and float(lv.grad.abs().max()) > 0 and np.abs(wl).max() > 0


def test_refusals_at_the_abi():
    lib = _C.load_library()
    N, C = 8, 3
    T = ref.layout(N)[2]
    x = torch.ones((6, T, C), device="cuda")
    y = torch.full((6, T, C), -7.0, device="cuda")
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    for fn in (lib.dm2_cube_prefilter, lib.dm2_cube_prefilter_backward):
        for args, text in (((1, N, C, -1, None, p(y)), b"null"), ((1, N, C, -1, p(x), None), b"null"),
                           ((1, N, 0, -1, p(x), p(y)), b"channels"), ((1, 0, C, -1, p(x), p(y)), b"at least 1"),
                           ((-1, N, C, -1, p(x), p(y)), b"number of cubes"), ((10923, N, C, -1, p(x), p(y)), b"number of cubes")):
            assert fn(*args, None) == 1 and text in lib.dm2_last_error(), (args, lib.dm2_last_error())
        torch.cuda.synchronize()
        assert (y == -7.0).all()                                          # a refused call writes nothing
        assert fn(1, 5, C, -1, None, None, None) == 0                     # T == 0: nothing runs
        assert fn(0, N, C, -1, None, None, None) == 0
        assert fn(10922, 5, C, -1, None, None, None) == 0                 # (the most cubes a call takes; T == 0)
        assert fn(1, N, C, 0, None, None, None) == 0                      # a limit of no levels
    # the limit is a word of its own: 1 builds level 1 alone, as r = 1
    T1 = ref.layout(N, 1)[2]
    x1 = torch.ones((6, T1, 1), device="cuda")
    y1 = torch.empty_like(x1)
    assert lib.dm2_cube_prefilter(1, N, 1, 1, p(x1), p(y1), None) == 0
    torch.cuda.synchronize()
    W, wb = ref.norm64(N, 1)
    assert (np.abs(_np(y1)[..., 0] - W) <= wb).all()
