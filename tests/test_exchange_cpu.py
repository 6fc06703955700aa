"""The sparse leaf-gradient exchange on the CPU: the numpy reference (tests/exchange_ref.py) against a float64 dense sum, and
sharding.reduce_leaves_sparse over gloo against the reference, bit for bit.  (The HIP kernels and sharding.DeviceExchange
are held to the same reference in tests/test_gpu_exchange.py.)"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import exchange_ref as xr
from util import ROOT  # noqa: F401  (puts the repository root on sys.path)
from dmesh2_renderer_amd.sharding import reduce_leaves_sparse


def _scene(seed, F, P, B, N, indexed=True):
    """-> faces, per-rank touched (B,F), per-rank flags, per-rank partials (random non-zero in every row)."""
    rng = np.random.RandomState(seed)
    faces = xr.indexed_faces(rng, F, P) if indexed else xr.soup_faces(F)
    touched = [xr.touched_pattern(rng, "random", B, F) for _ in range(N)]
    flags = [xr.mark(t, faces, P) for t in touched]
    parts = [xr.random_partials(rng, P, F, B) for _ in range(N)]
    return faces, touched, flags, parts


@pytest.mark.parametrize("F,P,B,N,indexed", [(500, 260, 2, 3, True), (100, 60, 1, 64, True), (2049, 1100, 1, 2, True),
                                             (64, 192, 3, 8, False), (333, 100, 4, 1, True)])
def test_reference_against_float64_dense_sum(F, P, B, N, indexed):
    """``reduce`` == the float64 sum of the flag-masked partials within (N - 1) 2^-24 sum_s |x_s| per element -- the bound of a
    sequential fp32 sum of N terms (N - 1 roundings, each at most 2^-24 of a partial sum that is at most sum |x_s|; the first
    add, to 0, is exact).  Rows no source flagged come out exactly 0 although every partial is non-zero there, and the
    slice-by-slice walk of the exchange gives the same bits as the dense walk."""
    faces, touched, flags, parts = _scene(100 + N, F, P, B, N, indexed)
    got = xr.reduce(parts, flags, N)
    for a, b in zip(got, xr.reduce_by_slices(parts, flags, N)):
        assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a, b)
    masks = [(fv[:, None], fv[:, None], ff, ff[None, :]) for ff, fv in flags]
    for i, name in enumerate(("dverts", "dcolor", "dopacity", "dintense")):
        terms = [np.where(m[i], p[i].astype(np.float64), 0.0) for p, m in zip(parts, masks)]
        want, mag = sum(terms), sum(np.abs(t) for t in terms)
        bound = (N - 1) * 2.0 ** -24 * mag
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), (name, float((err - bound).max()))
        nobody = ~np.any([np.broadcast_to(m[i], want.shape) for m in masks], axis=0)
        assert nobody.any() or N > 3, name                       # (up to three ranks leave rows that nobody flags)
        assert not got[i][nobody].any(), name
        assert all(p[i][nobody].all() for p in parts), name      # ... where every partial is non-zero


def test_reference_marks_counts_and_segments():
    """mark / counts / segments on a mesh small enough to state by hand: shared and unused vertices, P < F, N > rows."""
    faces = np.array([[0, 1, 2], [2, 1, 4], [4, 5, 0], [5, 5, 1], [7, 2, 0], [4, 2, 7], [1, 0, 5], [7, 7, 7]], np.int32)   # 3, 6 unused
    P, F, B, N = 8, 8, 2, 3
    touched = np.zeros((B, F), np.uint32); touched[0, 1] = 9; touched[1, 1] = 1; touched[1, 7] = 2
    ff, fv = xr.mark(touched, faces, P)
    assert ff.tolist() == [False, True, False, False, False, False, False, True]
    assert fv.tolist() == [False, True, True, False, True, False, False, True]
    assert xr.counts(ff, fv, N).tolist() == [[1, 2], [0, 1], [1, 1]]          # Fs = Ps = 3: owners of faces 1 | - | 7, verts 1 2 | 4 | 7
    rng = np.random.RandomState(0)
    part = xr.random_partials(rng, P, F, B)
    segs = xr.segments(ff, fv, N, *part)
    assert [(xr.row_ids(f).tolist(), xr.row_ids(v).tolist()) for f, v in segs] == [([1], [1, 2]), ([], [4]), ([7], [7])]
    assert segs[0][0].shape == (1, 2 + B) and segs[1][0].shape == (0, 2 + B) and segs[1][1].shape == (1, 7)
    assert np.array_equal(segs[2][0][0, 1:], [part[2][7], part[3][0, 7], part[3][1, 7]])
    assert np.array_equal(segs[0][1][1, 1:], np.concatenate([part[0][2], part[1][2]]))
    # nothing flagged, and more owners than rows: empty ranges stay empty
    none = xr.mark(np.zeros((B, F), np.uint32), faces, P)
    assert not xr.counts(*none, 64).any() and all(f.shape == (0, 2 + B) and v.shape == (0, 7) for f, v in xr.segments(*none, 64, *part))
    assert xr.counts(np.ones(F, bool), np.ones(P, bool), 64)[:, 0].tolist() == [1] * 8 + [0] * 56


# ---- sharding.reduce_leaves_sparse over gloo ----------------------------------------------------------------------------------
WORLD, GF, GP, GB, GSEED = 3, 500, 260, 2, 41


def _gloo_inputs(rank):
    """Rank's partials: random non-zero everywhere, then zero where the contract of reduce_leaves_sparse wants zeros (rows of
    faces outside ``touched`` and of vertices no touched face uses: those rows are not sent)."""
    faces, touched, flags, parts = _scene(GSEED, GF, GP, GB, WORLD)
    ff, fv = flags[rank]
    dv, dc, do, di = [x.copy() for x in parts[rank]]
    dv[~fv] = 0; dc[~fv] = 0; do[~ff] = 0; di[:, ~ff] = 0
    return faces, ff, (dv, dc, do, di)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        faces, ff, part = _gloo_inputs(rank)
        out = reduce_leaves_sparse(*[torch.from_numpy(x) for x in part], torch.from_numpy(faces), torch.from_numpy(ff))
        assert all(o.is_contiguous() for o in out)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **{f"o{i}": o.numpy() for i, o in enumerate(out)})
    finally:
        dist.destroy_process_group()


def test_reduce_leaves_sparse_over_gloo_equals_reference(tmp_path):
    """World 3, indexed mesh with shared and unused vertices, B = 2, overlapping random touched patterns: every rank ends
    with the reference's bits."""
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    ins = [_gloo_inputs(r) for r in range(WORLD)]
    flags = [xr.mark(i[1][None, :], i[0], GP) for i in ins]
    for r in range(WORLD):                      # (mark of the OR-ed faces gives back the flags the partials were zeroed by)
        assert np.array_equal(flags[r][0], ins[r][1])
    overlap = sum(f[0].astype(int) for f in flags)
    assert (overlap == WORLD).any() and (overlap == 0).any() and not sum(f[1].astype(int) for f in flags).all()
    want = xr.reduce([i[2] for i in ins], flags, WORLD)
    for r in range(WORLD):
        d = np.load(tmp_path / f"rank{r}.npz")
        for i, w in enumerate(want):
            assert d[f"o{i}"].dtype == np.float32 and d[f"o{i}"].shape == w.shape
            assert np.array_equal(d[f"o{i}"], w), (r, i)
