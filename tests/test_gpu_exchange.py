"""The device side of the sparse leaf-gradient exchange (csrc/dm2_exchange.hip: k_xchg_mark / _count / _pack / _unpack behind
_C.exchange_mark / _pack / _unpack; sharding.DeviceExchange) against the plain reference of tests/exchange_ref.py, exactly:
the exchange only copies rows and adds them in fp32 in source order, so every comparison is bit for bit.

N ranks are emulated on the one GPU with the all-to-all routed by hand.  A rank's touched pattern is not rendered but
injected: the face scratch of a cheap forward with the same (B, F) is filled with an int32 ramp, ``debug_fetch`` item 8 (the
accessor _C.touched_faces uses) then shows at which word of the buffer ``tiles_touched`` lies, and the pattern is written
there -- so indexed meshes, several views, any rank count and any flag density can be driven through ``exchange_mark`` without
restating the scratch layout.  The partial gradients are random non-zero in EVERY row, flagged or not."""
import os
import socket
import zlib

import numpy as np
import pytest
import torch

import exchange_ref as xr
from util import scenes, soup_args, to_dev

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _C():
    from dmesh2_renderer_amd import _C as c
    return c


# ---- a face scratch to inject into --------------------------------------------------------------------------------------------
def _face_scratch(B, F, P, faces_t):
    """The face scratch of a 16x16 forward over F faces in B views, every face beyond the depth range (culled)."""
    C = _C()
    f32 = torch.float32
    g = torch.Generator().manual_seed(B * 1000003 + F)
    z = lambda *s: torch.zeros(s, dtype=f32, device=DEV)                      # noqa: E731
    ndc = z(B, P, 3); ndc[..., 2] = 5.0
    img = (torch.rand((B, P, 2), generator=g) * 16).to(DEV)
    aa = lambda *s, dt=f32: torch.empty((B, 0) + s, dtype=dt, device=DEV)      # noqa: E731  (placeholders: tables_from_image)
    ray_d = z(B, 16, 16, 3); ray_d[..., 2] = 1.0
    args = (z(3), torch.zeros((B, 2), dtype=torch.int32, device=DEV), 16, 16, torch.randn((P, 3), generator=g).to(DEV), faces_t,
            z(P, 3) + 0.5, z(F) + 0.5, ndc, img, z(B, F) + 1.0, 1.0, aa(3, 2), aa(3, 2), aa(3, 2, dt=torch.bool), aa(3, 2), aa(3, 2),
            aa(3), 20, z(B, 16, 16, 3), ray_d)
    with C.tables_from_image(True):
        out = C.render_forward_cuda(*args)
    assert out[0] == 0
    return out[7]


def _inject(face_buf, touched_BF):
    """Write ``touched_BF`` (B, F) uint32 where the forward keeps tiles_touched; everything else of the buffer becomes 0."""
    C = _C()
    B, F = touched_BF.shape
    words = face_buf[: face_buf.numel() // 4 * 4].view(torch.int32)
    words.copy_(torch.arange(words.numel(), dtype=torch.int32, device=face_buf.device))
    probe = C.debug_fetch(8, B * F, 1, 0, face_buf, torch.int32, B * F)
    w = int(probe[0])
    assert torch.equal(probe, torch.arange(w, w + B * F, dtype=torch.int32, device=face_buf.device))
    words.zero_()
    words[w:w + B * F] = torch.from_numpy(touched_BF.reshape(-1).astype(np.int64).astype(np.int32)).to(face_buf.device)


_SCENES = {}


def _scene(F, P, mesh, B):
    """faces (numpy, torch), a face scratch, and one set of random partials (rolled per rank), shared by the densities."""
    key = (F, P, mesh, B)
    if key not in _SCENES:
        rng = np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)
        faces = xr.indexed_faces(rng, F, P) if mesh == "indexed" else xr.soup_faces(F)
        assert faces.shape == (F, 3) and faces.max() == P - 1
        if mesh == "indexed":
            assert np.unique(faces).size < P                      # vertices no face uses
        faces_t = torch.from_numpy(faces).to(DEV)
        _SCENES.clear()                                            # (one scene's buffers at a time)
        _SCENES[key] = (faces, faces_t, _face_scratch(B, F, P, faces_t), xr.random_partials(rng, P, F, B))
    return _SCENES[key]


def _partials(base, r):
    """Rank r's partials: the base rolled by an odd stride, so every row is non-zero and differs between ranks."""
    dv, dc, do, di = base
    k = 17 * r + 1
    return np.roll(dv, k, axis=0), np.roll(dc, 2 * k, axis=0), np.roll(do, k), np.roll(di, k, axis=1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# F, P, mesh, B, N
CASES = [(2049, 1100, "indexed", 1, 2),          # wave boundary + 1, P < F, slices not wave-aligned
         (4096, 12288, "soup", 1, 1),            # single owner, only full waves (unguarded flag loads only)
         (32769, 98307, "soup", 2, 3),           # second block, one id past the block edge
         (70001, 35200, "indexed", 3, 64),       # the most ranks, Fs = 1094: three owners in a wave
         (100, 60, "indexed", 1, 64),            # Fs = 2, Ps = 1: up to 50 owners in one wave, 14 owners with empty ranges
         (6149, 2047, "indexed", 4, 8)]          # widest row, P one short of a wave
DENSITIES = ["none", "all", "last", "random"]


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("F,P,mesh,B,N", CASES, ids=[f"F{c[0]}-P{c[1]}-{c[2]}-B{c[3]}-N{c[4]}" for c in CASES])
def test_exchange_kernels_equal_reference(F, P, mesh, B, N, density):
    """mark, count, pack and unpack of N emulated ranks: flags == mark, counts == counts, every segment sent == segments (ids as
    a set and value for value), and the assembled slices == reduce, all exactly."""
    C = _C()
    faces, faces_t, face_buf, base = _scene(F, P, mesh, B)
    rng = np.random.RandomState(zlib.crc32(repr((F, P, B, N, density)).encode()) & 0x7FFFFFFF)
    Fs, Ps = xr.slice_size(F, N), xr.slice_size(P, N)
    wf, wv = 2 + B, 7
    parts, flags, sends, cnts = [], [], [], []
    for r in range(N):
        touched = xr.touched_pattern(rng, density, B, F)
        _inject(face_buf, touched)
        fl, cnt = C.exchange_mark(face_buf, faces_t, B, P, N)
        ff, fv = xr.mark(touched, faces, P)
        fl_h = fl.cpu().numpy()
        assert fl.dtype == torch.uint8 and fl_h.shape == (F + P,)
        assert np.array_equal(fl_h[:F] != 0, ff) and np.array_equal(fl_h[F:] != 0, fv), r
        want_cnt = xr.counts(ff, fv, N)
        assert cnt.dtype == torch.int32 and np.array_equal(cnt.cpu().numpy(), want_cnt), r
        part = _partials(base, r)
        total = int((want_cnt[:, 0] * wf + want_cnt[:, 1] * wv).sum())
        send = C.exchange_pack(fl, cnt, total, *[torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in part])
        send_h = send.cpu().numpy()
        assert send_h.shape == (total,)
        off = 0
        for o, (want_f, want_v) in enumerate(xr.segments(ff, fv, N, *part)):
            nf, nv = want_cnt[o]
            fr = send_h[off:off + nf * wf].reshape(nf, wf); off += nf * wf
            vr = send_h[off:off + nv * wv].reshape(nv, wv); off += nv * wv
            assert np.array_equal(np.sort(xr.row_ids(fr)), xr.row_ids(want_f)), (r, o)
            assert np.array_equal(np.sort(xr.row_ids(vr)), xr.row_ids(want_v)), (r, o)
            assert np.array_equal(_bits(xr.sorted_rows(fr)), _bits(want_f)), (r, o)
            assert np.array_equal(_bits(xr.sorted_rows(vr)), _bits(want_v)), (r, o)
        assert off == total
        parts.append(part); flags.append((ff, fv)); sends.append(send); cnts.append(want_cnt)
    if density == "random" and N > 1:             # the ranks overlap: rows with several contributors
        assert (sum(f[0].astype(int) for f in flags) > 1).any()
    # the all-to-all, by hand: owner o receives, source by source, that source's segment for o
    ends = [np.concatenate([[0], np.cumsum(c[:, 0] * wf + c[:, 1] * wv)]) for c in cnts]
    sv, sf = [], []
    for o in range(N):
        rc = [cnts[s][o].tolist() for s in range(N)]
        recv = torch.cat([sends[s][ends[s][o]:ends[s][o + 1]] for s in range(N)])
        v, f = C.exchange_unpack(recv, rc, sum(a + b for a, b in rc), o, B, P, F)
        assert tuple(v.shape) == (Ps, 6) and tuple(f.shape) == (Fs, 1 + B)
        sv.append(v); sf.append(f)
    gv, gf = torch.cat(sv).cpu().numpy(), torch.cat(sf).cpu().numpy()
    assert not gv[P:].any() and not gf[F:].any()                   # the padding of the last slices, the empty owners
    got = (gv[:P, :3], gv[:P, 3:], gf[:F, 0], gf[:F, 1:].T)
    for name, a, w in zip(("dverts", "dcolor", "dopacity", "dintense"), got, xr.reduce(parts, flags, N)):
        assert a.shape == w.shape and np.array_equal(a, w), name


def _rows(ids, vals):
    return np.concatenate([np.asarray(ids, np.int32).view(np.float32)[:, None], np.asarray(vals, np.float32)], axis=1)


def test_unpack_ignores_rows_outside_the_owners_range():
    """A row whose id is not in [rank Fs, (rank + 1) Fs) (faces) or [rank Ps, (rank + 1) Ps) (vertices) changes nothing."""
    C = _C()
    B, P, F, N, rank = 2, 1000, 700, 3, 1
    Fs, Ps = xr.slice_size(F, N), xr.slice_size(P, N)             # 234, 334
    rng = np.random.RandomState(5)
    fid = np.array([Fs, Fs - 1, 2 * Fs - 1, 2 * Fs, 0, F - 1, Fs + 7, -1, -Fs, 2 ** 31 - 1, F + 5000], np.int64)
    vid = np.array([Ps - 1, Ps, 2 * Ps, 2 * Ps - 1, 0, P - 1, -1, Ps + 100, -(2 ** 31), 10 ** 6], np.int64)
    fr, vr = _rows(fid, rng.randn(fid.size, 1 + B)), _rows(vid, rng.randn(vid.size, 6))
    recv = torch.from_numpy(np.concatenate([fr.reshape(-1), vr.reshape(-1)])).to(DEV)
    rc = [[0, 0], [fid.size, vid.size], [0, 0]]
    sv, sf = C.exchange_unpack(recv, rc, fid.size + vid.size, rank, B, P, F)
    want_f, want_v = np.zeros((Fs, 1 + B), np.float32), np.zeros((Ps, 6), np.float32)
    for i, row in zip(fid, fr):
        if rank * Fs <= i < (rank + 1) * Fs:
            want_f[i - rank * Fs] = row[1:]
    for i, row in zip(vid, vr):
        if rank * Ps <= i < (rank + 1) * Ps:
            want_v[i - rank * Ps] = row[1:]
    assert np.count_nonzero(want_f.any(axis=1)) == 3 and np.count_nonzero(want_v.any(axis=1)) == 3
    assert np.array_equal(sf.cpu().numpy(), want_f) and np.array_equal(sv.cpu().numpy(), want_v)


def test_unpack_sums_one_id_from_every_source_in_source_order():
    """The same ids from all 64 sources, magnitudes spread over 2^-20 .. 2^20 so that any other order rounds differently."""
    C = _C()
    B, P, F, N, rank = 3, 64 * 5, 64 * 4, 64, 63                   # Fs = 4, Ps = 5: the last owner's ids
    rng = np.random.RandomState(6)
    fid, vid = np.array([255, 252]), np.array([319, 316, 315])
    chunks, want_f, want_v = [], np.zeros((4, 1 + B), np.float32), np.zeros((5, 6), np.float32)
    for s in range(N):
        fv = (rng.randn(fid.size, 1 + B) * 2.0 ** rng.randint(-20, 21, size=(fid.size, 1 + B))).astype(np.float32)
        vv = (rng.randn(vid.size, 6) * 2.0 ** rng.randint(-20, 21, size=(vid.size, 6))).astype(np.float32)
        order_f, order_v = rng.permutation(fid.size), rng.permutation(vid.size)        # (row order inside a segment is free)
        chunks += [_rows(fid[order_f], fv[order_f]).reshape(-1), _rows(vid[order_v], vv[order_v]).reshape(-1)]
        want_f[fid - rank * 4] = want_f[fid - rank * 4] + fv                            # fp32, one add per source
        want_v[vid - rank * 5] = want_v[vid - rank * 5] + vv
    recv = torch.from_numpy(np.concatenate(chunks)).to(DEV)
    sv, sf = C.exchange_unpack(recv, [[fid.size, vid.size]] * N, N * (fid.size + vid.size), rank, B, P, F)
    assert np.array_equal(sf.cpu().numpy(), want_f) and np.array_equal(sv.cpu().numpy(), want_v)
    backwards = np.zeros_like(want_f)                               # the test can tell orders apart
    for c in chunks[::-1][1::2]:
        rows = c.reshape(-1, 2 + B)
        backwards[xr.row_ids(rows) - rank * 4] += rows[:, 1:]
    assert not np.array_equal(backwards, want_f)


# ---- sharding.DeviceExchange end to end, one-rank RCCL group ---------------------------------------------------------------
def test_device_exchange_end_to_end_single_rank_rccl():
    """DeviceExchange(...).reduce(...) in a one-rank `nccl` group on an indexed mesh, B = 2, the pattern injected into a real
    forward's face scratch: flagged rows come back exactly, every other row 0 although the input is non-zero there, with the
    shapes and contiguity of reduce_leaves_sparse."""
    import torch.distributed as dist
    from dmesh2_renderer_amd.sharding import DeviceExchange, reduce_leaves_sparse
    C = _C()
    assert not dist.is_initialized()
    F, P, B = 5000, 2100, 2
    rng = np.random.RandomState(8)
    faces = xr.indexed_faces(rng, F, P)
    faces_t = torch.from_numpy(faces).to(DEV)
    face_buf = _face_scratch(B, F, P, faces_t)
    touched = xr.touched_pattern(rng, "random", B, F)
    _inject(face_buf, touched)
    ff, fv = xr.mark(touched, faces, P)
    part = xr.random_partials(rng, P, F, B)
    part_t = [torch.from_numpy(x).to(DEV) for x in part]
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        x = DeviceExchange(C, face_buf, faces_t, B, P)
        out = x.reduce(*part_t)
        masked = [part_t[0] * torch.from_numpy(fv).to(DEV)[:, None], part_t[1] * torch.from_numpy(fv).to(DEV)[:, None],
                  part_t[2] * torch.from_numpy(ff).to(DEV), part_t[3] * torch.from_numpy(ff).to(DEV)[None, :]]
        ref = reduce_leaves_sparse(*masked, faces_t, torch.from_numpy(ff).to(DEV))
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    want = xr.reduce([part], [(ff, fv)], 1)
    assert 0 < ff.sum() < F and 0 < fv.sum() < P
    for a, r, w, p, m in zip(out, ref, want, part, (fv[:, None], fv[:, None], ff, ff[None, :])):
        assert a.dtype == torch.float32 and a.shape == r.shape and a.stride() == r.stride() and a.is_contiguous()
        a = a.cpu().numpy()
        assert np.array_equal(a, w) and np.array_equal(r.cpu().numpy(), w)
        m = np.broadcast_to(m, p.shape)
        assert np.array_equal(_bits(a[m]), _bits(p[m])) and not a[~m].any() and p[~m].all()


# ---- the collectives a rank without a band issues ---------------------------------------------------------------------------
class _Work:
    def wait(self):
        return True


def _record_collectives(monkeypatch, world, rank, log):
    """Replace torch.distributed's collectives by stubs that note (op, dtype, numel, split sizes given?) and zero-fill their
    outputs: ONE process plays one rank of ``world`` at a time; nothing is sent anywhere."""
    import torch.distributed as dist

    def all_reduce(tensor, op=None, group=None, async_op=False):
        log.append(("all_reduce", tensor.dtype, tensor.numel(), False))
        return _Work() if async_op else None

    def all_to_all_single(output, input, output_split_sizes=None, input_split_sizes=None, group=None, async_op=False):
        assert (output_split_sizes is None) == (input_split_sizes is None)
        assert output.dtype == input.dtype
        log.append(("all_to_all_single", input.dtype, input.numel(), input_split_sizes is not None))
        output.zero_()
        return _Work() if async_op else None

    def all_gather_into_tensor(output, input, group=None, async_op=False):
        assert output.dtype == input.dtype and output.numel() == world * input.numel()
        log.append(("all_gather_into_tensor", input.dtype, input.numel(), False))
        output.zero_()
        return _Work() if async_op else None

    monkeypatch.setattr(dist, "get_world_size", lambda group=None: world)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: rank)
    monkeypatch.setattr(dist, "get_backend", lambda group=None: "nccl")
    monkeypatch.setattr(dist, "all_reduce", all_reduce)
    monkeypatch.setattr(dist, "all_to_all_single", all_to_all_single)
    monkeypatch.setattr(dist, "all_gather_into_tensor", all_gather_into_tensor)


@pytest.mark.parametrize("exchange", ["dense", "sparse"])
def test_rank_without_a_band_issues_its_peers_collectives(monkeypatch, exchange):
    """H = 16, world 2: one tile row, rank 0 has no band (band_rows -> 0 rows), rank 1 renders the frame.  Both must issue
    the same collectives in the same order with the same dtypes, and the same numel wherever the shapes fix it (the count
    exchange, the all-reduces, the all-gather; the payload all-to-all's size is data) -- anything else is a collective
    mismatch on RCCL: a hang, or garbage split sizes.  Played in one process with recording stubs; no multi-rank job."""
    from dmesh2_renderer_amd.sharding import BandShardedOp, band_rows
    W, H, F, world = 32, 16, 60, 2
    args, sc = soup_args(W, H, F, scenes.SEED_BASE + 77)
    dargs = to_dev(args)
    B, P = dargs[8].shape[0], dargs[4].shape[0]
    prep = (dargs[4], dargs[5], sc.mv[[0]].contiguous().to(DEV), sc.proj[[0]].contiguous().to(DEV), W, H)
    g = torch.Generator().manual_seed(1)
    dLc, dLd = torch.randn((B, H, W, 3), generator=g).to(DEV), torch.randn((B, H, W), generator=g).to(DEV)
    assert band_rows(H, world, 0)[1] == 0 and band_rows(H, world, 1) == (0, H)
    logs = []
    for rank in range(world):
        log = []
        with monkeypatch.context() as mp:
            _record_collectives(mp, world, rank, log)
            op = BandShardedOp(dargs, world, rank)
            op.forward()
            assert (op.fwd is None) == (rank == 0)
            out = op.backward_leaves(dLc[:, op.y0:op.y0 + op.rows].contiguous(), dLd[:, op.y0:op.y0 + op.rows].contiguous(), prep,
                                     exchange=exchange)
            torch.cuda.synchronize()
        assert [tuple(x.shape) for x in out] == [(P, 3), (P, 3), (F,), (B, F)]
        logs.append(log)
    fixed = [[(op_, dt, None if split else n) for op_, dt, n, split in log] for log in logs]
    assert fixed[0] == fixed[1], logs
    f32 = torch.float32
    if exchange == "dense":      # colour / opacity / intensity first (it overlaps the host-prep backward), then dverts
        assert fixed[1] == [("all_reduce", f32, 3 * P + F + B * F), ("all_reduce", f32, 3 * P)]
    else:
        Fs, Ps = xr.slice_size(F, world), xr.slice_size(P, world)
        assert fixed[1] == [("all_to_all_single", torch.int32, 2 * world), ("all_to_all_single", f32, None),
                            ("all_gather_into_tensor", f32, 6 * Ps + (1 + B) * Fs)]
        assert logs[0][1][2] == 0 and logs[1][1][2] > 0            # rank 0 sends nothing, rank 1 its touched rows
