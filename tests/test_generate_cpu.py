"""The scenes of tests/tet_scenes.py are what they claim, and the CPU oracle agrees with physics on them (no GPU needed).

Each scene exists for a branch of the tet walk that a jittered lattice seen from outside does not reach.  The properties are
measured on the oracle's own output (``oracle.cpu.generate_render_layers_cuda(..., return_first=True)`` and its binning);
why a walk ended comes from ``generate_ref.walk32``, a float32 numpy restatement of the walk that is first held to the oracle
bit for bit.  Every property has a floor well above zero (about a third of the measured value, given next to it), so that a
builder that silently stops producing its case fails here.
"""
import functools

import numpy as np
import pytest

import generate_ref as G
import tet_scenes as S
from util import scenes

L_ALL = 200             # above every walk's depth (asserted)


@functools.lru_cache(maxsize=None)
def _measured(name):
    ts, info = S.case(name)
    lr = S.renderer(ts)
    inp = G.inputs(lr, ts.verts, range(ts.mv.shape[0]))
    o = G.oracle(ts, inp, L_ALL)
    w = G.walk_scene(ts, inp, o, L_ALL)
    assert o["cnt"].max() < L_ALL
    assert np.array_equal(w["layers"], o["layers"]) and np.array_equal(w["cnt"], o["cnt"]), "walk32 is not the oracle's walk"
    assert not (w["cause"] == G.CAPPED).any() and not (w["cause"] == G.FULL).any()
    return ts, info, o, w


def _share(mask):
    return float(np.mean(mask))


def _report(name, **kv):
    print(f"{name}: " + ", ".join(f"{k} = {v:.4g}" for k, v in kv.items()))


def test_thresholds_are_read_from_the_sources():
    th = S.thresholds()
    assert 0 < th["LAY_CHUNK"] < th["TILE_SORT_RANK"] <= th["TILE_SORT_LDS"] < th["TILE_SORT_MAX"]


def test_aligned_rays_meet_vertices_and_edges():
    ts, info, o, w = _measured("aligned")
    c = w["cause"][0]                                                 # camera 0, whose rays the vertices sit on
    many, none = _share(c == G.NCAND2), _share(c == G.NCAND0)
    # the vertices on rays: the pixel's ray hits them within rounding (float64 distance of the fp32 vertex from the fp32 ray)
    lr = S.renderer(ts)
    on = np.nonzero(info["pixel_of"][:, 0] >= 0)[0]
    px, py = info["pixel_of"][on, 0], info["pixel_of"][on, 1]
    ro, rd = lr.ray_o[0].numpy().astype(np.float64)[py, px], lr.ray_d[0].numpy().astype(np.float64)[py, px]
    rd = rd / np.linalg.norm(rd, axis=-1, keepdims=True)               # (the rays are normalised with + 1e-6 on the length)
    d = ts.verts.numpy().astype(np.float64)[on] - ro
    dist = np.linalg.norm(d - (d * rd).sum(-1, keepdims=True) * rd, axis=-1)
    # central column / row: rays in the lattice planes x = 0 / y = 0
    W, H = ts.width, ts.height
    assert (lr.ray_d[0, :, W // 2, 0] == 0).all() and (lr.ray_d[0, H // 2, :, 1] == 0).all()
    in_plane = int((ts.verts.numpy()[:, 0] == 0).sum())
    _report("aligned", ncand_ge_2=many, ncand_0=none, vertices_on_rays=len(on), whole_columns=info["columns"],
            worst_distance=dist.max(), verts_in_plane_x0=in_plane)
    assert dist.max() <= 5e-7                                           # fp32 rounding of coordinates of magnitude 1
    assert len(on) >= 60 and info["columns"] >= 4 and in_plane >= 15      # measured 101, 8, 25
    assert many + none >= 0.04 and many >= 0.015 and none >= 0.02         # measured 0.112, 0.051, 0.061
    # the control: the same walk on the other camera, whose rays meet nothing, never ends this way
    c1 = w["cause"][1]
    assert _share((c1 == G.NCAND2) | (c1 == G.NCAND0)) < 0.002


def test_holes_orphans_cavities_and_one_tet_faces():
    ts, info, o, w = _measured("holes")
    ff, ft = o["ff"], o["ft"]
    have = ff >= 0
    f0 = np.where(have, ff, 0)
    orphan_first = have & info["orphan"][f0]
    assert not (o["cnt"][orphan_first] > 0).any() and (ft[orphan_first] == -1).all()       # a face was hit, the pixel is empty
    interior_one = have & info["one_tet"][f0] & ~info["hull"][f0]
    entered = interior_one & (ft >= 0)                                # met from the side without a tet: the walk enters
    from_tet_side = interior_one & (ft < 0)                           # met from the tet's side: nothing to enter
    cavity = (w["cause"] == G.LEFT) & ~info["hull"][w["last_face"]]   # left through a face that was interior: a cavity
    _report("holes", orphan_first_hits_cam0=orphan_first[0].sum(), orphan_first_hits_cam1=orphan_first[1].sum(),
            one_tet_entered=entered.sum(), one_tet_from_tet_side=from_tet_side.sum(), cavity_share_cam0=_share(cavity[0]),
            cavity_share_cam1=_share(cavity[1]), minus_one_slot0=int((ts.face_tets.numpy()[:, 0] < 0).sum()))
    assert orphan_first[0].sum() >= HOLES_FLOORS["orphan0"] and orphan_first[1].sum() >= HOLES_FLOORS["orphan1"]
    assert entered.sum() >= HOLES_FLOORS["entered"] and from_tet_side.sum() >= HOLES_FLOORS["tet_side"]
    assert _share(cavity[0]) >= HOLES_FLOORS["cavity0"] and _share(cavity[1]) >= HOLES_FLOORS["cavity1"]
    ftn = ts.face_tets.numpy()
    assert ((ftn[:, 0] < 0) & (ftn[:, 1] >= 0)).sum() >= 100 and ((ftn[:, 0] >= 0) & (ftn[:, 1] < 0)).sum() >= 100


# measured: 1927, 903, 1572, 1653 pixels of 6300 per camera; 0.373, 0.572
HOLES_FLOORS = dict(orphan0=600, orphan1=300, entered=500, tet_side=500, cavity0=0.12, cavity1=0.19)


def test_inside_cameras_and_the_plan_cull():
    ts, info, o, w = _measured("inside")
    F, bn = ts.faces.shape[0], o["bn"]
    out = {}
    for cam in (0, 1):
        st = S.straddlers(ts, cam)
        touched = bn.tiles_touched[cam * F:(cam + 1) * F]
        out[cam] = (int(st.sum()), int((st & (touched == 0)).sum()), int((st & (touched > 0)).sum()))
    hit = _share(o["cnt"] > 0)
    _report("inside", straddlers_cam0=out[0][0], culled_cam0=out[0][1], kept_cam0=out[0][2], straddlers_cam1=out[1][0],
            culled_cam1=out[1][1], kept_cam1=out[1][2], pixels_with_layers=hit)
    for cam in (0, 1):
        assert out[cam][0] >= 100 and out[cam][1] >= 4 and out[cam][2] >= 80        # measured 428 / 12 / 416 and 270 / 11 / 259
    assert hit >= 0.5
    # an inside camera's first hit is seen from within: the tet the walk enters is not always face_tets' first entry
    ff, ft = o["ff"], o["ft"]
    m = (ff >= 0) & (ft >= 0)
    second = ts.face_tets.numpy()[ff[m], 1] == ft[m]
    assert 0.1 <= second.mean() <= 0.9


def test_flat_tets_and_zero_area_faces():
    ts, info, o, w = _measured("flat")
    nn, vol = S.face_normal_norms(ts), S.tet_volumes(ts)
    ref_vol = S.tet_volumes(scenes.tet_lattice(ts.width, ts.height, 5, seed=0, jitter=0.0))
    flipped = _share(np.sign(vol) != np.sign(ref_vol))
    clamped = nn < np.float32(1e-4)
    # the clamped faces that walks actually stand in front of: faces of visited tets
    seen = np.zeros(len(nn), bool)
    seen[ts.tet_faces.numpy()[w["visited"]].reshape(-1)] = True
    back, none = _share(w["cause"] == G.BACK), _share(w["cause"] == G.NCAND0)
    _report("flat", clamped_faces=clamped.sum(), zero_normal_faces=(nn == 0).sum(), clamped_faces_walked=(clamped & seen).sum(),
            inverted_tets=flipped, near_flat_tets=_share(np.abs(vol) < 1e-4), ended_backfacing=back, ended_ncand_0=none)
    assert (nn == 0).sum() >= 12 and (clamped & seen).sum() >= 6
    assert flipped >= 0.05 and _share(np.abs(vol) < 1e-4) >= 0.015
    assert back >= 0.1 and none >= 0.005                               # measured 0.34, 0.016


FLOORS_DUP = (900, 300, 0.03)


def test_duplicates_decide_first_hits_by_list_order():
    ts, info, o, w = _measured("duplicates")
    ff = o["ff"]
    have = ff >= 0
    f0 = np.where(have, ff, 0)
    dup_first = have & info["dup"][f0]
    # equal keys, equal t, a strict compare: the lower id, first in the list, is the first hit -- never the copy
    assert not (have & (f0 >= info["copy"][0])).any()
    orphaned_original = np.zeros(len(info["dup"]), bool)
    orphaned_original[info["src"][info["real"]]] = True
    blind = have & orphaned_original[f0]                               # the first hit is the original, the mesh's face is the copy
    assert (o["cnt"][blind] == 0).all()
    lost = _share(w["cause"] == G.CNT)                                  # standing on a face its tet does not list
    _report("duplicates", first_hits_on_a_duplicated_face=dup_first.sum(), first_hits=have.sum(), emptied_by_an_orphan_original=blind.sum(),
            ended_cnt_not_3=lost)
    assert dup_first.sum() >= FLOORS_DUP[0] and blind.sum() >= FLOORS_DUP[1] and lost >= FLOORS_DUP[2]
    # copies of both kinds are crossed mid-walk too
    listed = np.unique(o["layers"][o["layers"] >= 0])
    assert (listed >= info["copy"][0]).sum() >= 20


@pytest.mark.parametrize("name", ["deep", "deep_sort"])
def test_deep_lists(name):
    ts, info, o, w = _measured(name)
    th = S.thresholds()
    lens = G.list_lengths(o["bn"])
    pos = G.list_positions(o["bn"], o["ff"])
    chunk0, later = int(((pos >= 0) & (pos < th["LAY_CHUNK"])).sum()), int((pos >= th["LAY_CHUNK"]).sum())
    _report(name, shortest_list=lens.min(), longest_list=lens.max(), first_hits_in_chunk_0=chunk0, first_hits_in_later_chunks=later,
            deepest_first_hit=pos.max(), deepest_walk=o["cnt"].max())
    assert (o["ff"] >= 0).all()
    if name == "deep":
        assert lens.min() >= 8 * th["LAY_CHUNK"]                       # EVERY tile: several chunks (measured 9835 = 38 chunks)
        assert th["TILE_SORT_LDS"] < lens.max() <= th["TILE_SORT_MAX"]
        assert chunk0 >= 150 and later >= 150                          # measured 529 and 495 of 1024
    else:
        assert lens.max() > th["TILE_SORT_MAX"]                        # the plan's global-sort route (measured 51038)
        assert chunk0 >= 60 and later >= 250                           # measured 199 and 825
    assert pos.max() >= 2 * th["LAY_CHUNK"]


@pytest.mark.parametrize("name", ["chunk_edge", "chunk_edge3"])
def test_chunk_edge_last_entry_is_the_first_hit(name):
    ts, info, o, w = _measured(name)
    lens = G.list_lengths(o["bn"])
    pos = G.list_positions(o["bn"], o["ff"])
    chunk = S.thresholds()["LAY_CHUNK"]
    assert lens.tolist() == [info["entries"]] and info["entries"] % chunk == 1
    assert (o["ff"] == info["back"]).all() and (pos == info["entries"] - 1).all()       # all 256 pixels: the last chunk's only entry
    assert (o["ft"] == 0).all() and (o["cnt"] >= 1).all() and (o["cnt"] == 2).mean() > 0.8  # into the tet, out by a side face


@pytest.mark.parametrize("name", ["aligned", "holes", "duplicates"])
@pytest.mark.parametrize("table", ["zeros", "ones", "odd"])
def test_existence_tables(name, table):
    """All 0: nothing listed, whatever was crossed.  All 1 and values other than 0 / 1: any non-zero flag counts, so a table
    of 2, -1, INT_MIN gives what the same table squashed to 0 / 1 gives."""
    ts, info = S.case(name)
    tab = S.existence_tables(ts.faces.shape[0], 11)[table]
    lr = S.renderer(ts)
    inp = G.inputs(lr, ts.verts, [0])
    o = G.oracle(ts, inp, 4, existence=tab)
    if table == "zeros":
        assert not o["cnt"].any() and (o["layers"] == -1).all()
    else:
        squashed = G.oracle(ts, inp, 4, existence=(tab != 0).astype(np.int32))
        assert np.array_equal(o["layers"], squashed["layers"]) and np.array_equal(o["cnt"], squashed["cnt"])
        assert (o["cnt"] > 0).mean() > 0.2
    if table == "odd":
        assert all((tab == v).sum() > 0 for v in S.ODD_VALUES)


BRUTE = [(4, 70, "own"), (4, 70, "odd"), (4, 70, "ones"), (5, 72, "own")]


@pytest.mark.parametrize("n,seed,table", BRUTE)
def test_oracle_against_float64_brute_force(n, seed, table):
    """Hole-free jittered lattices (test_generate_is_a_prefix's image, cameras and L): the oracle's layers are the existing
    faces each ray hits, ordered by t, up to the face the ray leaves the mesh through, cut at L -- by a float64 brute force
    that knows no tiles, tets or walk.  Excused: near-ties along the ray and barycentrics within the margin of an edge,
    capped at 0.1 % of the pixels."""
    ts, inp, tab = brute_case(n, seed, table)
    br8 = G.brute64(ts.verts, ts.faces, tab, inp["ro"], inp["rd"], 8, hull=S.hull_faces(ts))
    for L in (8, 2):
        o = G.oracle(ts, inp, L, existence=tab)
        br = G.cut(br8, L)
        G.check_brute(o["layers"], o["cnt"], br, f"oracle, tet_lattice(n={n}), existence {table}, L={L}")
        assert (br["cnt"] > 0).mean() > 0.3


def brute_case(n, seed, table, lr=None):
    W, H, bidx = 96, 72, [1, 0]
    ts = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + seed, num_cams=2)
    tab = ts.faces_existence.numpy() if table == "own" else S.existence_tables(ts.faces.shape[0], seed)[table]
    lr = lr or S.renderer(ts)
    verts = ts.verts.to(lr.ray_o.device)
    return ts, G.inputs(lr, verts, bidx), tab
