"""The per-slot ops at the launch-time regimes no op file enters (tests/launch_regimes.py has the census and the parameter lists;
DESIGN.md 8, "Launch regimes and who tests them"): the forwards' sweeps with more channel groups than lanes, deep and fine hash
grids, and the grids' bounds on views, textures and tile rows, at the bound and one step past it.

Every comparison is the op file's own: its reference module through its ``_check_*`` helpers where it has them, else the lines
of its tests (forwards bit-equal to the forward32 restatement, gradients under GRAD_TOL or util.summation_bound as that file
holds them).  Nothing here states a tolerance of its own."""
import contextlib

import numpy as np
import pytest
import torch

import bary_derivatives_ref as bref
import composite_ref as cref
import coverage_ref as cvref
import hash_grid_ref as href
import launch_regimes as lr
import rasterize_ref as rref
import shading_ref as sref
import test_gpu_bary_derivatives as tgb
import test_gpu_composite as tgcomp
import test_gpu_coverage_op as tgcov
import test_gpu_hash_grid as tgh
import test_gpu_interpolate as tgi
import test_gpu_shading as tgs
import test_gpu_texture as tgt
import test_gpu_texture_cube as tgc
import test_gpu_texture_cube_mip as tgcm
import test_gpu_texture_mip as tgm
import test_gpu_texture_volume as tgv
import texture_mip_ref as mref
from util import GRAD_TOL, rel_linf, summation_bound, watch_rel_linf

from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

f32 = np.float32
PATTERN = 0x7FC0DEAD                             # a NaN no kernel writes: an output that keeps it was not touched


@contextlib.contextmanager
def _watch(mod, shifted_C=None):
    """The checks of the op file ``mod`` observed: seen["rel"] collects every util.rel_linf they compute, and the file's WORST
    (the files that hold util.summation_bound keep one) starts empty and is put back afterwards, merged.  With ``shifted_C``
    the file's uploads (its ``_cu``) of float32 arrays of that many channels become views 4 bytes into their storage: no 16-byte
    alignment, so the launchers take their scalar paths (seen["shifted"]: how many uploads; the caller asserts that there were
    some)."""
    seen = {"shifted": 0}
    real_cu = mod._cu

    def cu(a):
        if a is None or a.dtype != np.float32 or a.ndim < 2 or a.shape[-1] != shifted_C:
            return real_cu(a)
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = real_cu(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        seen["shifted"] += 1
        return v
    before = dict(getattr(mod, "WORST", {}))
    if shifted_C is not None:
        mod._cu = cu
    if hasattr(mod, "WORST"):
        mod.WORST.clear()
    try:
        with watch_rel_linf() as rel:
            seen["rel"] = rel
            yield seen
    finally:
        mod._cu = real_cu
        if hasattr(mod, "WORST"):
            for k, v in before.items():
                mod.WORST[k] = max(mod.WORST.get(k, 0.0), v)


def _report(what, mod, seen, relative=None):
    """The worst error / bound of the checks just run: the file's own WORST where it holds util.summation_bound per element,
    the worst util.rel_linf over GRAD_TOL where it holds relative L-inf (``relative``: whether it does; by default, whether
    the file imports rel_linf).  A file that should have computed one and did not fails here."""
    ratios = dict(getattr(mod, "WORST", {}))
    if hasattr(mod, "rel_linf") if relative is None else relative:
        assert seen["rel"], (what, "no relative error was computed")
        ratios["rel L-inf / GRAD_TOL"] = max(seen["rel"]) / GRAD_TOL
    assert ratios, what
    print(what, "forward bit-equal; worst err / bound", ratios)
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)


def _long(shape):
    """The rows bound's shape: one view of 2^20 - 16 slots, every one with an upstream gradient.  Its tables are larger than the
    other cases' (64 x 64 texels, 16 x 16 a cube face, 2048 attribute rows, 4096 faces), so that an element of a table's gradient
    sums about a thousand terms, as in the op files' own cases, and not 10^5."""
    return shape[0] == 1 and int(np.prod(shape)) >= 1 << 15


def _ids(rng, shape, hi=9):
    """ids with -1 in one slot of six (one slot: live)."""
    rl = rng.integers(0, hi, shape).astype(np.int32)
    if rl.size > 1:
        rl[rng.uniform(size=shape) < 1 / 6] = -1
    return rl


# ---- one adapter per op: inputs(rng, shape, C, per_view) -> args; forward(args, what) over every mode; grads(args, g, what) -------
class _Texture:
    mod, name, entry = tgt, "texture", "dm2_texture"

    def inputs(self, rng, shape, C, per_view):
        return dict(uv=rng.uniform(-2, 3, shape + (2,)).astype(f32), rl=_ids(rng, shape), tex=tgt._tex(rng, shape[0], (64, 64) if _long(shape) else (5, 3), C, per_view))

    def forward(self, a, what, every=True):
        for m in tgt.MODES if every else tgt.MODES[:1]:
            tgt._check_forward(a["uv"], a["tex"], a["rl"], *m, what + m)

    def grads(self, a, g, what):
        tgt._check_grads(a["uv"], a["tex"], a["rl"], "linear", "wrap", g, what)

    def shim(self, a):
        return _C.texture_cuda(tgt._cu(a["uv"]), tgt._cu(a["tex"]), tgt._cu(a["rl"]))

    def abi(self, shape, a, out, g, grads):
        B, H, W, L = shape
        p = _C._ptr
        Ht, Wt = (int(n) for n in a["tex"].shape[-3:-1])
        return ((B, H, W, L, Ht, Wt, 1, 0, 1, 0, p(a["rl"]), p(a["uv"]), p(a["tex"]), p(out), None),
                (B, H, W, L, Ht, Wt, 1, 0, 1, 0, p(a["rl"]), p(a["uv"]), p(a["tex"]), p(g), p(grads[0]), p(grads[1]), None))


class _Cube:
    mod, name, entry = tgc, "texture_cube", "dm2_texture_cube"

    def inputs(self, rng, shape, C, per_view):
        return dict(d=rng.standard_normal(shape + (3,)).astype(f32), rl=_ids(rng, shape), tex=tgc._tex(rng, shape[0], 16 if _long(shape) else 3, C, per_view))

    def forward(self, a, what, every=True):
        for m in tgc.ref.FILTERS if every else ("linear",):
            tgc._check_forward(a["d"], a["tex"], a["rl"], m, what + (m,))

    def grads(self, a, g, what):
        tgc._check_grads(a["d"], a["tex"], a["rl"], "linear", g, what)

    def shim(self, a):
        return _C.texture_cube_cuda(tgc._cu(a["d"]), tgc._cu(a["tex"]), tgc._cu(a["rl"]))

    def abi(self, shape, a, out, g, grads):
        B, H, W, L = shape
        p = _C._ptr
        N = int(a["tex"].shape[-2])
        return ((B, H, W, L, N, 1, 0, 1, p(a["rl"]), p(a["d"]), p(a["tex"]), p(out), None),
                (B, H, W, L, N, 1, 0, 1, p(a["rl"]), p(a["d"]), p(a["tex"]), p(g), p(grads[0]), p(grads[1]), None))


class _CubeMip:
    mod, name, entry = tgcm, "texture_cube_mip", "dm2_texture_cube_mip"
    N = 4                                                                     # a chain of three levels
    N_AT_BOUNDS = 1                                                           # (the reference of a chain over 2^20 slots takes 8 s)

    def inputs(self, rng, shape, C, per_view):
        N = self.N if int(np.prod(shape)) < 1 << 15 else self.N_AT_BOUNDS
        d = (rng.standard_normal(shape + (3,)) * np.exp(rng.uniform(-2, 2, shape + (1,)))).astype(f32)
        lod = rng.uniform(-1, 4, shape).astype(f32)
        tex, mip = tgcm._cube(rng, shape[0], N, C, per_view)
        return dict(d=d, lod=lod, rl=_ids(rng, shape), tex=tex, mip=mip)

    def forward(self, a, what, every=True):
        tgcm._check_forward(a["d"], a["lod"], a["tex"], a["mip"], a["rl"], None, what)

    def grads(self, a, g, what):
        tgcm._check_grads(a["d"], a["lod"], a["tex"], a["mip"], a["rl"], None, g, what)

    def shim(self, a):
        return _C.texture_cube_mip_cuda(*(tgcm._cu(a[k]) for k in ("d", "lod", "tex", "mip", "rl")), None)

    def abi(self, shape, a, out, g, grads):
        B, H, W, L = shape
        p = _C._ptr
        head = (B, H, W, L, int(a["tex"].shape[-2]), 1, 0, -1, p(a["rl"]), p(a["d"]), p(a["lod"]), p(a["tex"]), p(a["mip"]))
        return head + (p(out), None), head + (p(g), p(grads[0]), p(grads[1]), p(grads[2]), None)


class _Volume:
    mod, name, entry = tgv, "texture_volume", "dm2_texture_volume"

    def inputs(self, rng, shape, C, per_view):
        return dict(p=rng.uniform(-0.4, 1.4, shape + (3,)).astype(f32), rl=_ids(rng, shape), grid=tgv._grid(rng, shape[0], 3, C, per_view))

    def forward(self, a, what, every=True):
        for f, b in [(f, b) for f in tgv.ref.FILTERS for b in tgv.ref.BOUNDARIES] if every else [("linear", "clamp")]:
            tgv._check_forward(a["p"], a["grid"], a["rl"], f, b, what + (f, b))

    def grads(self, a, g, what):
        tgv._check_grads(a["p"], a["grid"], a["rl"], "linear", "clamp", g, what)

    def shim(self, a):
        return _C.texture_volume_cuda(tgv._cu(a["p"]), tgv._cu(a["grid"]), tgv._cu(a["rl"]))

    def abi(self, shape, a, out, g, grads):
        B, H, W, L = shape
        p = _C._ptr
        return ((B, H, W, L, 3, 1, 0, 1, 1, p(a["rl"]), p(a["p"]), p(a["grid"]), p(out), None),
                (B, H, W, L, 3, 1, 0, 1, 1, p(a["rl"]), p(a["p"]), p(a["grid"]), p(g), p(grads[0]), p(grads[1]), None))


class _Mip:
    mod, name, entry = tgm, "texture_mip", "dm2_texture_mip"
    size = (16, 8)                                                            # four levels

    def inputs(self, rng, shape, C, per_view):
        if _long(shape):                      # footprints up to four texels of 64 x 64: levels 0 .. 3, the coarsest of them 8 x 8
            size = (64, 64)
            uv, da, rl = rng.uniform(-0.5, 1.5, shape + (2,)).astype(f32), mref.footprints(rng, shape, *size, -2.0, 2.0), _ids(rng, shape)
        else:
            size = self.size
            uv, da, rl = mref.case(shape, *size, seed=int(rng.integers(1 << 30)))
        tex = rng.standard_normal(((shape[0],) if per_view else ()) + size + (C,), dtype=f32)
        return dict(uv=uv, da=da, rl=rl, tex=tex, mip=mref.mipmaps(tex))

    def forward(self, a, what, every=True):
        for b in mref.BOUNDARIES if every else ("wrap",):
            tgm._check(a["uv"], a["da"], a["tex"], a["mip"], a["rl"], b, None, None, what + (b,))

    def grads(self, a, g, what):
        tgm._check(a["uv"], a["da"], a["tex"], a["mip"], a["rl"], "wrap", None, g, what)

    def shim(self, a):
        return _C.texture_mip_cuda(*(tgm._cu(a[k]) for k in ("uv", "da", "tex", "mip", "rl")), "wrap", None)

    def abi(self, shape, a, out, g, grads):
        B, H, W, L = shape
        p = _C._ptr
        head = (B, H, W, L, *(int(n) for n in a["tex"].shape[-3:-1]), 1, 0, 0, -1, p(a["rl"]), p(a["uv"]), p(a["da"]), p(a["tex"]), p(a["mip"]))
        return head + (p(out), None), head + (p(g), p(grads[0]), p(grads[1]), p(grads[2]), None)


class _Interpolate:
    mod, name, entry = tgi, "interpolate", "dm2_interpolate"
    F, N = 20, 15

    def inputs(self, rng, shape, C, per_view):
        F, N = (4096, 2048) if _long(shape) else (self.F, self.N)
        return dict(rl=_ids(rng, shape, F), bary=rng.uniform(0, 1, shape + (3,)).astype(f32),
                    attr=tgi._attr(rng, shape[0], N, C, per_view), af=rng.integers(0, N, (F, 3)).astype(np.int32))

    def forward(self, a, what, every=True):
        tgi._check_forward(a["rl"], a["bary"], a["attr"], a["af"], what)

    def grads(self, a, g, what):
        tgi._check_grads(a["rl"], a["bary"], a["attr"], a["af"], g, what)

    def shim(self, a):
        return _C.interpolate_cuda(*(tgi._cu(a[k]) for k in ("rl", "bary", "attr", "af")))

    def abi(self, shape, a, out, g, grads):
        B, H, W, L = shape
        p = _C._ptr
        head = (B, H, W, L, int(a["af"].shape[0]), int(a["attr"].shape[-2]), 1, 0, p(a["rl"]), p(a["bary"]), p(a["attr"]), p(a["af"]))
        return head + (p(out), None), head + (p(g), p(grads[0]), p(grads[1]), None)


OPS = {op.name: op for op in (_Interpolate(), _Texture(), _Mip(), _Cube(), _CubeMip(), _Volume())}
assert tuple(OPS) == lr.WIDE_OPS and set(lr.SLOT_GRID_OPS) == set(OPS)


# ---- wide channels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", lr.SCALAR_CS + lr.VECTOR_CS)
@pytest.mark.parametrize("name", lr.WIDE_OPS)
def test_wide_channels(name, C):
    """259 slots in one view (a full block and a ragged one of 3) with a shared table, and two views with a table each, some
    slots empty: every mode of the forward, and both gradients of the linear filter at one boundary mode, at a channel count whose
    sweep takes another regime than any C <= 33 (lr.sweep_regime); C = 256 from tables 4 bytes into their storage (the scalar
    path), every other multiple of 4 aligned (the vector path)."""
    op = OPS[name]
    shifted = (C, True) in lr.wide_cases(name)
    print(name, "C", C, "CV", lr.wide_cv(name, C, shifted), "sweep regime:", lr.sweep_regime(lr.wide_cv(name, C, shifted)))
    rng = np.random.default_rng(1000 + C)
    with _watch(op.mod, C if shifted else None) as seen:
        for shape in lr.WIDE_SHAPES:
            a = op.inputs(rng, shape, C, per_view=shape[0] > 1)
            assert (a["rl"] < 0).any() and (a["rl"] >= 0).any()
            g = rng.standard_normal(shape + (C,), dtype=f32)
            what = (name, C, shape)
            op.forward(a, what)
            op.grads(a, g, what)
        assert (seen["shifted"] > 0) == shifted
        _report((name, C), op.mod, seen)


# ---- hash grids -----------------------------------------------------------------------------------------------------------------
def _hash_case(case):
    N, q, NL, lg, Fs = lr.HASH_CASES[case]
    R, dense = lr.hash_levels(N, q, NL, lg)
    assert R == href.resolutions(NL, N, q) and [bool(dense >> v & 1) for v in range(NL)] == [href.is_dense(r, 1 << lg) for r in R]
    return N, q, NL, 1 << lg, Fs, R, dense


def _hash_check(what, p, table, rl, N, q, modes, g):
    with _watch(tgh) as seen:
        for f, b in modes:
            tgh._check_forward(p, table, rl, N, q, f, b, what + (f, b))
        dt, dp = tgh._check_grads(p, table, rl, N, q, "linear", modes[-1][1], g, what)
        _report(what, tgh, seen)
    return dt, dp


ALL_MODES = tuple((f, b) for f in href.FILTERS for b in href.BOUNDARIES)


@pytest.mark.parametrize("case,F", [(c, F) for c in ("32 levels", "32 levels, 17 dense", "32 levels, all dense", "workload")
                                    for F in lr.HASH_CASES[c][4]])
def test_hash_grid_levels(case, F):
    """Deep grids: 32 levels (dense word 0x1, 0x1FFFF, 0xFFFFFFFF) and the 16 levels of the layout the op was added for, on the
    259-slot shape (the small tables on the two-view shape as well)."""
    N, q, NL, T, _, R, dense = _hash_case(case)
    print(case, "F", F, "resolutions", R, "dense word", hex(dense), "T", T)
    rng = np.random.default_rng(2000 + NL + F)
    table = tgh._table(rng, NL, T, F)
    for shape in lr.WIDE_SHAPES[:2 if T <= 1 << 15 else 1]:
        p = rng.uniform(-0.4, 1.4, shape + (3,)).astype(f32)
        rl = _ids(rng, shape)
        g = rng.standard_normal(shape + (NL * F,), dtype=f32)
        _, dp = _hash_check((case, F, shape), p, table, rl, N, q, ALL_MODES, g)
        assert np.abs(dp).max() > 0


@pytest.mark.parametrize("boundary_mode", href.BOUNDARIES)
@pytest.mark.parametrize("case", ["finest 2^20", "finest 2^19, 2^20"])
def test_hash_grid_finest_level_at_its_limit(case, boundary_mode):
    """R = 2^20 at the finest level, positions over [-15.9, 15.9]^3: x R - 0.5 up to the 2^24 rule, and per axis its two fp32
    neighbours, x = 16 - 2^-20 (live) and x = 16 (empty); -16 as well.  hash_grid_ref.empty says which is which."""
    N, q, NL, T, (F,), R, dense = _hash_case(case)
    assert R[-1] == 1 << 20 and dense == 0
    shape = lr.WIDE_SHAPES[0]
    rng = np.random.default_rng(2100 + NL)
    p = rng.uniform(-15.9, 15.9, shape + (3,)).astype(f32)
    flat = p.reshape(-1, 3)
    below, at = f32(16.0) - f32(2.0 ** -20), f32(16.0)
    assert below < at and np.nextafter(below, f32(np.inf), dtype=f32) == at
    edge = []
    for axis in range(3):
        for k, v in enumerate((below, at, -below, -at)):
            flat[20 * axis + 3 * k + 1, axis] = v
            edge.append((20 * axis + 3 * k + 1, k))
    empty = href.empty(p, R).reshape(-1)
    for s, k in edge:                                                         # the reference decides; 16 - 2^-20 is live and 16 is not
        print("slot", s, "coordinate", flat[s].tolist(), "empty" if empty[s] else "live")
        assert k > 1 or bool(empty[s]) == (k == 1), (s, k)
    assert 3 <= empty.sum() <= 12 and (~empty).sum() >= 259 - 12
    table = tgh._table(rng, NL, T, F)
    g = rng.standard_normal(shape + (NL * F,), dtype=f32)
    modes = tuple((f, boundary_mode) for f in href.FILTERS)
    _, dp = _hash_check((case, boundary_mode), p, table, None, N, q, modes, g)
    assert not dp.reshape(-1, 3)[empty].any()


@pytest.mark.parametrize("case", ["2^24 rows, dense", "2^24 rows, hashed"])
def test_hash_grid_largest_table(case):
    """log2(T) = 24, one level, F = 1: 64 MB of table and as much gradient for 259 slots.  Every row no live slot reads holds NaN
    (as test_gpu_hash_grid.py's poisoned table); the gradient is held per element over the whole table, exact zeros where no
    term arrives."""
    N, q, NL, T, (F,), R, dense = _hash_case(case)
    assert T == 1 << 24 and dense == (1 if R[0] ** 3 == T else 0)
    shape = lr.WIDE_SHAPES[0]
    rng = np.random.default_rng(2200 + N)
    p = rng.uniform(-0.2, 1.2, shape + (3,)).astype(f32)
    rl = _ids(rng, shape)
    g = rng.standard_normal(shape + (F,), dtype=f32)
    for boundary_mode in href.BOUNDARIES:
        read = np.zeros(T, bool)
        for f in href.FILTERS:
            st = href.stage(p, R, T, rl, f, boundary_mode)
            read[st["rows"][0][~st["empty"]].reshape(-1)] = True
        table = np.full((1, T, F), np.nan, f32)
        table[0, read] = rng.standard_normal((int(read.sum()), F), dtype=f32) + 10
        assert 259 < read.sum() < 10 * 259
        dt, dp = _hash_check((case, boundary_mode), p, table, rl, N, q, tuple((f, boundary_mode) for f in href.FILTERS), g)
        assert not dt[0, ~read].any() and np.abs(dp).max() > 0


# ---- the bounds -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["views", "rows"])
@pytest.mark.parametrize("name", lr.SLOT_GRID_OPS)
def test_at_the_bound(name, which):
    """B = 65535 with a table per view and H = W = L = 1, and B = 1 with H = 16 * 65535 (65535 tile rows), one channel: forward and
    both gradients against the op file's reference."""
    op = OPS[name]
    shape = lr.AT_BOUND[which == "rows"]
    assert shape[0] == lr.MAX_VIEWS or (shape[1] + 15) // 16 == 65535
    rng = np.random.default_rng(3000 + len(name))
    with _watch(op.mod) as seen:
        a = op.inputs(rng, shape, 1, per_view=shape[0] > 1)
        g = rng.standard_normal(shape + (1,), dtype=f32)
        op.forward(a, (name, which), every=False)
        op.grads(a, g, (name, which))
        _report((name, which), op.mod, seen)


def _pattern(*shape):
    return torch.full(shape, PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(t):
    return bool((t.view(torch.int32) == PATTERN).all())


def _refused(lib, entry, args, outs, what):
    assert getattr(lib, entry)(*args) == 1, what
    msg = lib.dm2_last_error().decode()
    torch.cuda.synchronize()
    assert all(_untouched(o) for o in outs), (what, "an output was written")
    return msg


@pytest.mark.parametrize("which", ["views", "rows"])
@pytest.mark.parametrize("name", lr.SLOT_GRID_OPS)
def test_one_step_past_the_bound(name, which):
    """B = 65536 and H = 16 * 65535 + 1: the shim raises with the op's message, the C entries return 1 and the outputs handed to
    them keep the pattern they were filled with (nothing was launched).  The inputs have their full sizes."""
    op = OPS[name]
    shape = lr.PAST_BOUND[which == "rows"]
    rng = np.random.default_rng(3100)
    a = op.inputs(rng, shape, 1, per_view=False)
    lib = _C.load_library()
    word = "texture" if name == "texture_mip" else name                      # (the mip op's slot check is dm2_texture's)
    with pytest.raises(RuntimeError, match=rf"{word}: too many slots, rows or views"):
        op.shim(a)
    dev = {k: op.mod._cu(v) for k, v in a.items()}
    out, g = _pattern(*shape, 1), torch.zeros(shape + (1,), device="cuda")
    grads = [_pattern(4 * int(np.prod(shape)) + 1024) for _ in range(3)]      # each at least as long as any gradient of the op
    fwd, bwd = op.abi(shape, dev, out, g, grads)
    for entry, args, outs in ((op.entry, fwd, [out]), (op.entry + "_backward", bwd, grads)):
        msg = _refused(lib, entry, args, outs, (name, which, entry))
        assert msg == f"{word}: too many slots, rows or views", msg


def _hash_inputs(rng, shape, NL, F, T):
    return rng.uniform(-0.2, 1.2, shape + (3,)).astype(f32), _ids(rng, shape), tgh._table(rng, NL, T, F)


@pytest.mark.parametrize("which", ["views", "rows"])
def test_hash_grid_at_the_bound(which):
    """B * NL = 65535 as 4369 views of 15 levels, and 65535 tile rows at one level, F = 1."""
    B, H, W, L, NL = lr.HASH_AT_BOUND[which == "rows"]
    assert B * NL == 65535 or (H + 15) // 16 == 65535
    rng = np.random.default_rng(3200)
    p, rl, table = _hash_inputs(rng, (B, H, W, L), NL, 1, 16)
    g = rng.standard_normal((B, H, W, L, NL), dtype=f32)
    _hash_check(("hash_grid", which), p, table, rl, 2, 17, (("nearest", "wrap"), ("linear", "clamp")), g)


@pytest.mark.parametrize("which", ["views", "rows"])
def test_hash_grid_one_step_past_the_bound(which):
    B, H, W, L, NL = lr.HASH_PAST_BOUND[which == "rows"]
    assert B * NL == 65536 or (H + 15) // 16 == 65536
    shape = (B, H, W, L)
    rng = np.random.default_rng(3300)
    p, rl, table = (tgh._cu(x) for x in _hash_inputs(rng, shape, NL, 1, 16))
    with pytest.raises(RuntimeError, match="hash_grid: too many slots, rows or views"):
        _C.hash_grid_cuda(p, table, rl, 2, 17 / 16, "linear", "clamp")
    lib = _C.load_library()
    out, g = _pattern(*shape, NL), torch.zeros(shape + (NL,), device="cuda")
    dt, dp = _pattern(NL, 16, 1), _pattern(*shape, 3)
    ptr = _C._ptr
    head = (B, H, W, L, 2, 4, NL, 1, 17, 1, 1, ptr(rl), ptr(p), ptr(table))
    assert _refused(lib, "dm2_hash_grid", head + (ptr(out), None), [out], which) == "hash_grid: too many slots, rows or views"
    assert _refused(lib, "dm2_hash_grid_backward", head + (ptr(g), ptr(dt), ptr(dp), None), [dt, dp], which) == \
        "hash_grid: too many slots, rows or views"


# ---- composite: its forward is flat over the pixels, the per-face alpha's backward one block per tile and view ---------------------
def _composite_case(rng, shape, per_face, F):
    """composite_ref.case's recipe at ``shape`` = (B, H, W, L), one channel."""
    rl = rng.integers(0, F, shape).astype(np.int32)
    rl[rng.uniform(size=shape) < 0.2] = -1
    alpha = cref._alphas(rng, (F,) if per_face else shape, shape[3])
    c = dict(values=rng.standard_normal(shape + (1,), dtype=f32), alpha=alpha, render_layers=rl, background=rng.uniform(0, 1, 1).astype(f32),
             g=rng.standard_normal(shape[:3] + (1,), dtype=f32), gA=rng.standard_normal(shape[:3], dtype=f32))
    c["out"], c["final_T"], c["n_contrib"], c["blend"] = cref.forward32(c["values"], alpha, rl, c["background"], full=True)
    return c


@pytest.mark.parametrize("per_face", [False, True])
@pytest.mark.parametrize("which", ["views", "rows"])
def test_composite_at_the_bound(which, per_face):
    shape = lr.AT_BOUND[which == "rows"][:3] + (2,)
    c = _composite_case(np.random.default_rng(3400 + per_face), shape, per_face, 4096 if _long(shape) else 211)
    with _watch(tgcomp) as seen:
        tgcomp._check_forward(c, ("composite", which, per_face))
        tgcomp._check_grads(c, ("composite", which, per_face))
        _report(("composite", which, per_face), tgcomp, seen)


@pytest.mark.parametrize("which", ["views", "rows"])
def test_composite_one_step_past_the_bound(which):
    shape = lr.PAST_BOUND[which == "rows"]
    B, H, W, L = shape
    lib, ptr = _C.load_library(), _C._ptr
    for per_face in (False, True):
        c = _composite_case(np.random.default_rng(3500), shape, per_face, 211)
        v, a, rl, bg = tgcomp._inputs(c)
        with pytest.raises(RuntimeError, match="composite: too many pixels, rows or views"):
            _C.composite_cuda(v, a, rl, bg)
        outs = [_pattern(B, H, W, 1), _pattern(B, H, W), _pattern(B, H, W), _pattern(B, H, W)]
        head = (B, H, W, L, 1, 211 if per_face else 0, int(per_face), ptr(v), ptr(a), ptr(rl), ptr(bg))
        msg = _refused(lib, "dm2_composite", head + (ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3].view(torch.int32)), None), outs, which)
        assert msg == "composite: too many pixels, rows or views"
        grads = [_pattern(B, H, W, L, 1), _pattern(B, H, W, L)]
        n, g, gA = tgcomp._cu(c["n_contrib"]), tgcomp._cu(c["g"]), tgcomp._cu(c["gA"])
        msg = _refused(lib, "dm2_composite_backward", head + (ptr(n), ptr(g), ptr(gA), ptr(grads[0]), ptr(grads[1]), None), grads, which)
        assert msg == "composite: too many pixels, rows or views"


# ---- coverage: tile_grid(W, H, B) forward and backward -------------------------------------------------------------------------------
def _coverage_case(rng, shape):
    """Views bound: a triangle of its own per view over the view's one pixel, three slots in four empty.  Rows bound: 64 triangles
    spread over the 2^20 - 16 rows of the one-pixel-wide frame, the first and the last tile row among them, each listed in the
    eleven rows around it (some of which it misses); every other slot empty."""
    B, H, W, L = shape
    rl = np.full(shape, -1, np.int32)
    if B > 1:
        vi = rng.uniform(-1.0, 2.0, (B, 3, 2)).astype(f32)
        fc = np.array([[0, 1, 2]], np.int32)
        rl[rng.uniform(size=shape) < 0.25] = 0
    else:
        F = 64
        ys = np.linspace(3, H - 4, F).astype(np.int64)
        tri = rng.uniform(-1.0, 2.0, (F, 3, 2))
        tri[..., 1] = ys[:, None] + rng.uniform(-3.0, 4.0, (F, 3))
        vi = tri.reshape(1, 3 * F, 2).astype(f32)
        fc = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
        for k, y in enumerate(ys):
            rl[0, max(y - 5, 0):y + 6, 0, 0] = k
        assert rl[0, :16].max() >= 0 and rl[0, -16:].max() >= 0
    return dict(render_layers=rl, verts_image=vi, faces=fc, g=cvref.upstream(shape, 7))


@pytest.mark.parametrize("which", ["views", "rows"])
def test_coverage_at_the_bound(which):
    """Forward bit-equal to coverage32 through the C entry and the shim, dL/dverts_image within GRAD_TOL of grad_image64 with exact
    zeros where the reference has them, as tests/test_gpu_coverage_op.py holds them."""
    shape = lr.AT_BOUND[which == "rows"]
    c = _coverage_case(np.random.default_rng(3600), shape)
    rl, vi, fc = c["render_layers"], c["verts_image"], c["faces"]
    with watch_rel_linf() as rel:
        for t in (1.0, 0.5):
            info = cvref.coverage32(rl, vi, fc, t)
            assert info["partial"].sum() > 50 and info["empty"].any()
            for got in (tgcov._raw_forward(c, t), _C.coverage_cuda(tgcov._cu(rl), tgcov._cu(vi), tgcov._cu(fc), t).cpu().numpy()):
                assert np.array_equal(tgcov._bits(got), tgcov._bits(info["cov"])), (which, t, int((tgcov._bits(got) != tgcov._bits(info["cov"])).sum()))
            want = cvref.grad_image64(rl, vi, fc, t, c["g"], info)
            got = tgcov._backward(c, t, c["g"])
            assert got.shape == want.shape and np.isfinite(got).all() and want.any()
            assert not got[want == 0].any(), (which, t)
            assert rel_linf(got, want) <= GRAD_TOL, (which, t)
    print(("coverage", which), "forward bit-equal; worst err / bound", {"rel L-inf / GRAD_TOL": max(rel) / GRAD_TOL})


@pytest.mark.parametrize("which", ["views", "rows"])
def test_coverage_one_step_past_the_bound(which):
    shape = lr.PAST_BOUND[which == "rows"]
    B, H, W, L = shape
    rl = torch.zeros(shape, dtype=torch.int32, device="cuda")
    vi, fc = torch.rand((B, 3, 2), device="cuda"), torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda")
    g = torch.ones(shape, device="cuda")
    for call in (lambda: _C.coverage_cuda(rl, vi, fc, 1.0), lambda: _C.coverage_backward_cuda(rl, vi, fc, 1.0, g)):
        with pytest.raises(RuntimeError, match="coverage: too many rows or views"):
            call()
    lib, ptr = _C.load_library(), _C._ptr
    out, dvi = _pattern(*shape), _pattern(B, 3, 2)
    head = (B, H, W, L, 3, 1, 1.0, None, ptr(rl))
    assert _refused(lib, "dm2_coverage", head + (None, ptr(vi), ptr(fc), ptr(out), None), [out], which) == "coverage: too many rows or views"
    assert _refused(lib, "dm2_coverage_backward", head + (ptr(vi), ptr(fc), ptr(g), ptr(dvi), None), [dvi], which) == \
        "coverage: too many rows or views"


# ---- shading_vectors and bary_derivatives: flat grids per view, the view on the grid's z ------------------------------------------
def _shading_case(rng, B):
    shape = (B, 1, 1, 1)
    rl = _ids(rng, shape)
    t = np.where(rl >= 0, rng.uniform(0.5, 5.0, shape), -1.0).astype(f32)
    rd = rng.standard_normal((B, 1, 1, 3))
    rd = (rd / np.linalg.norm(rd, axis=-1, keepdims=True)).astype(f32)
    return dict(layers=rl, t=t, normals=(rng.standard_normal(shape + (3,)) * rng.uniform(0.25, 3.0, shape + (1,))).astype(f32),
                ro=rng.standard_normal((B, 1, 1, 3)).astype(f32), rd=rd)


def test_shading_vectors_at_the_bound():
    """65535 views of one pixel: the four outputs bit-equal to shading_ref.forward32, both gradients per element within
    util.summation_bound of grads64 with exact zeros where no term arrives, as tests/test_gpu_shading.py holds them."""
    rng = np.random.default_rng(3700)
    c = _shading_case(rng, lr.MAX_VIEWS)
    args = tuple(tgs._cu(c[k]) for k in ("layers", "t", "normals", "ro", "rd"))
    tgs._same(_C.shading_vectors_cuda(*args), sref.forward32(c["layers"], c["t"], c["normals"], c["ro"], c["rd"]), "views")
    gs = [rng.standard_normal(c["normals"].shape).astype(f32) for _ in range(3)]
    dt, dn = _C.shading_vectors_backward_cuda(*args, *(tgs._cu(g) for g in gs), True, True)
    wt, wn, st, sn = sref.grads64(c["layers"], c["t"], c["normals"], c["ro"], c["rd"], *gs)
    live, ratios = c["layers"] >= 0, {}
    for name, got, want, sabs in (("t", dt, wt, st), ("normals", dn, wn, sn)):
        got = tgs._np(got).astype(np.float64)
        assert np.isfinite(got).all() and not got[~live].any() and not got[sabs == 0].any() and np.abs(want).max() > 0
        bound = summation_bound(np.abs(want).max(), sabs)
        ratios[name] = float((np.abs(got - want) / bound).max())
        assert (np.abs(got - want) <= bound).all(), name
    print(("shading_vectors", "views"), "forward bit-equal; worst err / bound", ratios)


def test_shading_vectors_one_step_past_the_bound():
    B = lr.MAX_VIEWS + 1
    c = _shading_case(np.random.default_rng(3701), B)
    rl, t, nr, ro, rd = (tgs._cu(c[k]) for k in ("layers", "t", "normals", "ro", "rd"))
    g = torch.ones((B, 1, 1, 1, 3), device="cuda")
    for call in (lambda: _C.shading_vectors_cuda(rl, t, nr, ro, rd), lambda: _C.shading_vectors_backward_cuda(rl, t, nr, ro, rd, g, g, g, True, True)):
        with pytest.raises(RuntimeError, match="shading_vectors: too many slots or views"):
            call()
    lib, ptr = _C.load_library(), _C._ptr
    outs = [_pattern(B, 1, 1, 1, 3) for _ in range(4)]
    head = (B, 1, 1, 1, 0, None, ptr(rl), ptr(t), ptr(nr), ptr(ro), ptr(rd), None)
    assert _refused(lib, "dm2_shading_vectors_window", head + tuple(ptr(o) for o in outs) + (None,), outs, "views") == \
        "shading_vectors: too many slots or views"
    grads = [_pattern(B, 1, 1, 1), _pattern(B, 1, 1, 1, 3)]
    assert _refused(lib, "dm2_shading_vectors_backward_window", head + (ptr(g), ptr(g), ptr(g), ptr(grads[0]), ptr(grads[1]), None), grads,
                    "views") == "shading_vectors: too many slots or views"


def _bary_case(rng, B):
    """The soup scene's mesh and cameras (its three views, repeated), a frame of one pixel per view, random ids."""
    s = rref.scene("soup")
    cam = bref.camera_block(*bref.scene_cameras("soup"))
    cam = np.ascontiguousarray(cam[np.arange(B) % cam.shape[0]])
    layers = rng.integers(-1, s["faces"].shape[0], (B, 1, 1, 1)).astype(np.int32)
    return layers, s["verts"], s["faces"], cam


def test_bary_derivatives_at_the_bound():
    """65535 views of one pixel, bit-equal to bary_derivatives_ref.forward32 (the op has no backward)."""
    layers, verts, faces, cam = _bary_case(np.random.default_rng(3800), lr.MAX_VIEWS)
    got = _C.bary_derivatives_cuda(tgb._cu(layers), tgb._cu(verts), tgb._cu(faces), tgb._cu(cam))
    want = bref.forward32(layers, verts, faces, cam, 1, 1)
    tgb._same(got, want, "views")
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0 and not got[0].cpu().numpy()[layers < 0].any()
    print(("bary_derivatives", "views"), "forward bit-equal")


def test_bary_derivatives_one_step_past_the_bound():
    B = lr.MAX_VIEWS + 1
    layers, verts, faces, cam = (tgb._cu(x) for x in _bary_case(np.random.default_rng(3801), B))
    with pytest.raises(RuntimeError, match="bary_derivatives: too many slots or views"):
        _C.bary_derivatives_cuda(layers, verts, faces, cam)
    lib, ptr = _C.load_library(), _C._ptr
    outs = [_pattern(B, 1, 1, 1, 3) for _ in range(2)]
    args = (B, 1, 1, 1, verts.shape[0], faces.shape[0], None, ptr(layers), ptr(verts), ptr(faces), ptr(cam), ptr(outs[0]), ptr(outs[1]), None)
    assert _refused(lib, "dm2_bary_derivatives_window", args, outs, "views") == "bary_derivatives: too many slots or views"


# ---- texture_mipmaps: tex_flat_grid(n, NB), the textures on the grid's y ----------------------------------------------------------
def test_texture_mipmaps_at_the_bound():
    """65535 textures of 2 x 2: the chain bit-equal to texture_mip_ref.mipmaps, its gradient within GRAD_TOL of mipmaps_backward64,
    as tests/test_gpu_texture_mip.py::test_chain_forward_and_backward holds them."""
    rng = np.random.default_rng(3900)
    tex = rng.standard_normal((lr.MAX_VIEWS, 2, 2, 1), dtype=f32)
    want = mref.mipmaps(tex)
    mip = _C.texture_mipmaps_cuda(tgm._cu(tex))
    assert tuple(mip.shape) == want.shape and np.array_equal(tgm._bits(tgm._np(mip)), tgm._bits(want))
    g = rng.standard_normal(want.shape, dtype=f32)
    back = mref.mipmaps_backward64(tex.shape, None, g)
    with watch_rel_linf() as rel:
        assert np.abs(back).max() > 0 and rel_linf(tgm._np(_C.texture_mipmaps_backward_cuda(tgm._cu(tex), None, tgm._cu(g))), back) <= GRAD_TOL
    print(("texture_mipmaps", "views"), "forward bit-equal; worst err / bound", {"rel L-inf / GRAD_TOL": max(rel) / GRAD_TOL})


def test_texture_mipmaps_one_step_past_the_bound():
    NB = lr.MAX_VIEWS + 1
    tex, g = torch.zeros((NB, 2, 2, 1), device="cuda"), torch.ones((NB, 1, 1), device="cuda")
    for call in (lambda: _C.texture_mipmaps_cuda(tex), lambda: _C.texture_mipmaps_backward_cuda(tex, None, g)):
        with pytest.raises(RuntimeError, match=r"texture_mip: the number of textures must lie in \[0, 65535\]"):
            call()
    lib, ptr = _C.load_library(), _C._ptr
    mip, dtex = _pattern(NB, 1, 1), _pattern(NB, 2, 2, 1)
    msg = "texture_mip: the number of textures must lie in [0, 65535]"
    assert _refused(lib, "dm2_texture_mipmaps", (NB, 2, 2, 1, -1, ptr(tex), ptr(mip), None), [mip], "textures") == msg
    assert _refused(lib, "dm2_texture_mipmaps_backward", (NB, 2, 2, 1, -1, ptr(g), ptr(dtex), None), [dtex], "textures") == msg
