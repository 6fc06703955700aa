"""A plain numpy statement of the sparse leaf-gradient exchange (dmesh2_renderer_amd.sharding.reduce_leaves_sparse,
sharding.DeviceExchange, csrc/dm2_exchange.hip): no torch.distributed, no GPU.

Ids are owned by contiguous ranges: id i of n belongs to owner i // ceil(n / N).  A rank sends every owner the rows of the
faces its band touched (in any view) and of their vertices; an owner starts its slice at 0 and adds what arrives source by
source, 0 .. N-1, in fp32; the slices, concatenated and cut to P / F, are the result on every rank.  Every add is a plain fp32
add of two numbers, so the product must agree with ``reduce`` bit for bit."""
import numpy as np


def slice_size(n, N):
    return -(-int(n) // int(N))


def mark(touched_BF, faces, P):
    """touched_BF (B, F), any integer or bool type (non-zero = the face was binned in that view); faces (F, 3) ->
    (flag_f (F) bool, flag_v (P) bool): the OR over the views, and the vertices of the flagged faces."""
    flag_f = (np.asarray(touched_BF) != 0).any(axis=0)
    flag_v = np.zeros(int(P), dtype=bool)
    flag_v[np.asarray(faces, dtype=np.int64)[flag_f].reshape(-1)] = True
    return flag_f, flag_v


def counts(flag_f, flag_v, N):
    """-> (N, 2) int64: [face rows, vertex rows] this rank sends to every owner."""
    out = np.zeros((N, 2), dtype=np.int64)
    for k, fl in enumerate((flag_f, flag_v)):
        if fl.size:
            out[:, k] = np.bincount(np.nonzero(fl)[0] // slice_size(fl.size, N), minlength=N)[:N]
    return out


def segments(flag_f, flag_v, N, dverts, dcolor, dopacity, dintense):
    """-> per owner (face rows (nf, 2 + B) float32 [id | dopacity | dintense(B)], vertex rows (nv, 7) float32 [id | dverts(3) |
    dcolor(3)]), ids ascending, the id's int32 bits in the float slot.  (The order inside a segment is free in the product:
    compare after sorting by id.)"""
    F, P = flag_f.size, flag_v.size
    Fs, Ps = slice_size(F, N), slice_size(P, N)
    fid, vid = np.nonzero(flag_f)[0], np.nonzero(flag_v)[0]
    frow = np.concatenate([fid.astype(np.int32).view(np.float32)[:, None], np.asarray(dopacity, np.float32)[fid][:, None],
                           np.asarray(dintense, np.float32)[:, fid].T], axis=1)
    vrow = np.concatenate([vid.astype(np.int32).view(np.float32)[:, None], np.asarray(dverts, np.float32)[vid],
                           np.asarray(dcolor, np.float32)[vid]], axis=1)
    cf, cv = np.searchsorted(fid, np.arange(N + 1) * Fs), np.searchsorted(vid, np.arange(N + 1) * Ps)      # (ids ascend)
    return [(frow[cf[o]:cf[o + 1]], vrow[cv[o]:cv[o + 1]]) for o in range(N)]


def row_ids(rows):
    return np.ascontiguousarray(rows[:, 0]).view(np.int32).astype(np.int64)


def sorted_rows(rows):
    return rows[np.argsort(row_ids(rows), kind="stable")]


def reduce(partials_per_rank, flags_per_rank, N):
    """partials_per_rank[s] = (dverts (P,3), dcolor (P,3), dopacity (F), dintense (B,F)) of source s, flags_per_rank[s] =
    (flag_f, flag_v) -> dense float32 (dverts, dcolor, dopacity, dintense): zeros, then the flagged rows of every source
    added in source order in fp32 (within a source the ids are distinct, so the fancy-indexed add is one add per element)."""
    assert len(partials_per_rank) == N and len(flags_per_rank) == N
    P, F, B = partials_per_rank[0][0].shape[0], partials_per_rank[0][2].shape[0], partials_per_rank[0][3].shape[0]
    dv, dc = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32)
    do, di = np.zeros((F,), np.float32), np.zeros((B, F), np.float32)
    for (pv, pc, po, pi), (ff, fv) in zip(partials_per_rank, flags_per_rank):
        fid, vid = np.nonzero(ff)[0], np.nonzero(fv)[0]
        dv[vid] = dv[vid] + np.asarray(pv, np.float32)[vid]
        dc[vid] = dc[vid] + np.asarray(pc, np.float32)[vid]
        do[fid] = do[fid] + np.asarray(po, np.float32)[fid]
        di[:, fid] = di[:, fid] + np.asarray(pi, np.float32)[:, fid]
    return dv, dc, do, di


def reduce_by_slices(partials_per_rank, flags_per_rank, N):
    """The same sum, walked the way the exchange moves it: every owner's slice (padded to ceil(n / N) rows, starting at 0)
    receives the segments of sources 0 .. N-1 in turn, and the slices are concatenated and cut to P / F."""
    P, F, B = partials_per_rank[0][0].shape[0], partials_per_rank[0][2].shape[0], partials_per_rank[0][3].shape[0]
    Fs, Ps = slice_size(F, N), slice_size(P, N)
    segs = [segments(ff, fv, N, *p) for p, (ff, fv) in zip(partials_per_rank, flags_per_rank)]
    sv, sf = np.zeros((N, Ps, 6), np.float32), np.zeros((N, Fs, 1 + B), np.float32)
    for o in range(N):
        for s in range(N):
            fr, vr = segs[s][o]
            fi, vi = row_ids(fr) - o * Fs, row_ids(vr) - o * Ps
            sf[o, fi] = sf[o, fi] + fr[:, 1:]
            sv[o, vi] = sv[o, vi] + vr[:, 1:]
    gv, gf = sv.reshape(N * Ps, 6)[:P], sf.reshape(N * Fs, 1 + B)[:F]
    return gv[:, :3].copy(), gv[:, 3:].copy(), gf[:, 0].copy(), gf[:, 1:].T.copy()


# ---- scenes of the tests ---------------------------------------------------------------------------------------------------
def indexed_faces(rng, F, P, unused=0.1):
    """(F, 3) int32 faces over P vertices of which about ``unused`` appear in no face, the others in several (F > P / 3);
    vertex P - 1 is always used (the last id is the edge of the vertex loops)."""
    used = np.nonzero(rng.rand(P) >= unused)[0]
    used = np.union1d(used, [P - 1])
    faces = used[rng.randint(0, used.size, size=(F, 3))]
    faces[-1, 2] = P - 1
    return faces.astype(np.int32)


def soup_faces(F):
    return np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def touched_pattern(rng, density, B, F):
    """(B, F) uint32 tiles-touched words: "none", "all", "last" (the last face alone, in the last view alone) or "random"
    (~30 % per rank, spread over the views, plus every 7th face on every rank so that ranks overlap)."""
    t = np.zeros((B, F), dtype=np.uint32)
    if density == "all":
        t[:] = rng.randint(1, 1000, size=(B, F))
    elif density == "last":
        t[B - 1, F - 1] = 3
    elif density == "random":
        on = rng.rand(F) < 0.3
        on[::7] = True
        view = rng.randint(0, B, size=F)                     # the view that saw the face; some faces are seen by every view
        every = rng.rand(F) < 0.2
        for b in range(B):
            t[b] = np.where(on & ((view == b) | every), rng.randint(1, 1000, size=F), 0)
    else:
        assert density == "none", density
    return t


def random_partials(rng, P, F, B):
    """Random normal fp32 in EVERY row: a row that should not travel must not show up."""
    return (rng.randn(P, 3).astype(np.float32), rng.randn(P, 3).astype(np.float32), rng.randn(F).astype(np.float32),
            rng.randn(B, F).astype(np.float32))
