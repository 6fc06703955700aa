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


DEEP_SORT_SIZE = (16, 16)        # deep_sort's image in the rasterize tests: one tile that lists every face of the lattice


def _tet_size(name):
    return DEEP_SORT_SIZE if name == "deep_sort" else (None, None)


@pytest.mark.parametrize("name", ref.SCENES + ref.TET_CASES)
def test_early_exit_changes_no_list(name):
    """The kernel's depth stop (a face whose min depth lies beyond the largest max depth of a full set of held hits cannot
    come nearer) leaves every list of every scene the GPU tests use as the contract defines it, for every L they use -- the
    tet scenes included, whose rays lie in face planes (the hit rule keeps their noise t out of the lists) and whose camera
    sits inside the mesh."""
    tet = name in ref.TET_CASES
    s = ref.tet_case(name, *_tet_size(name)) if tet else ref.scene(name)
    stopped = 0
    for exist in (None, "fe"):
        if tet:
            x = ref.tet_intersect(name, exist, True, *_tet_size(name))
        else:
            x = ref.intersect(s["W"], s["H"], s["verts"], s["faces"], None if exist is None else s[exist], s["verts_ndc"],
                              s["verts_image"], s["ray_o"], s["ray_d"])
        for L in (1, 4, 16, 17, 40) if tet else (1, 3, 8, 16, 17, 40):
            want = ref.select(x, L)
            got = ref.select(x, L, early_exit=True)
            for k in ("layers", "cnt", "bary", "t"):
                assert np.array_equal(got[k], want[k]), (name, exist, L, k, int((got[k] != want[k]).sum()))
            stopped += int((want["cnt"] == L).sum())
    if name != "no_faces":
        assert stopped > 0                                          # (full lists: the stop had a chance to act)


def test_early_exit_needs_the_hit_rule_on_aligned():
    """Without the rule (``rule=False``) the same walk leaves the contract on ``aligned``: a phantom hit's t has nothing to do
    with its face's depth range, which the stop relies on.  (What the rule is for; measured 106 / 68 / 18 pixels at L = 1 / 4 /
    17.)"""
    x = ref.tet_intersect("aligned", None, False)
    differ = {L: int((ref.select(x, L)["layers"] != ref.select(x, L, early_exit=True)["layers"]).any(-1).sum()) for L in (1, 4, 17)}
    print(f"aligned without the hit rule: pixels whose early-exit list differs {differ}")
    assert all(v > 0 for v in differ.values())


@pytest.mark.parametrize("name", ref.SCENES)
def test_hit_rule_changes_no_ordinary_list(name):
    """On soup, lattice and degenerate (and no_faces) the rule removes no hit: old and new ``hits32`` agree everywhere."""
    s = ref.scene(name)
    a = (s["W"], s["H"], s["verts"], s["faces"], None, s["verts_ndc"], s["verts_image"], s["ray_o"], s["ray_d"])
    old, new = ref.intersect(*a, rule=False), ref.intersect(*a)
    assert np.array_equal(old["hit"], new["hit"]), ref.rule_removed(old, new)
    if name != "no_faces":
        assert old["hit"].sum() > 5000


@pytest.mark.parametrize("name", ["aligned", "inside", "holes", "flat", "duplicates", "deep"])
def test_hits_against_float64_brute_force(name):
    """Every hit of the restatement against float64 Moeller-Trumbore over ALL faces (nothing read from the binning).
    Soundness: every hit has float64 barycentrics > -1e-4 and |t - t64| <= 1e-4 t + 1e-5.  Completeness: every clear hit
    (``clear_hits64``: |cos| > 1e-3, barycentrics > 1e-4, t > 1e-4, depth cull, existence, no camera-plane straddler) is a
    hit, and for L = 1, 4, 16 every clear hit nearer than a full list's last t is listed.  Zero failures, nothing excused."""
    s = ref.tet_case(name)
    every = ref.clear_hits64(s)
    for exist in (None, "fe_odd"):
        x = ref.tet_intersect(name, exist)
        bad = ref.unsound64(s, x)
        clear = every if exist is None else tuple(a[s[exist][every[1]] != 0] for a in every)    # (existence not 0)
        missing = {L: len(ref.missing64(x, clear, L)) for L in (None, 1, 4, 16)}
        print(f"{name} existence {exist}: {int(x['hit'].sum())} hits, {int(bad.sum())} unsound; {len(clear[0])} clear hits, missing {missing}")
        assert len(clear[0]) > 0.5 * x["hit"].sum() > 1000
        assert not bad.any(), np.argwhere(bad)[:5]
        assert not any(missing.values()), missing


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


# ---- reach: each tet scene takes the branch it was built for.  Floors: about a third of the figure measured with the hit rule
# in (the convention of test_generate_cpu.py: it survives a change of seed). -------------------------------------------------------
FLOORS = dict(aligned_edge_hits=1100, aligned_edge_pixels=150, aligned_ties_L4=60, aligned_ties_15_16=14, aligned_ties_31_32=2,
              aligned_removed_hits=190, aligned_removed_pixels=85, duplicates_ties_L4=2300, duplicates_ties_15_16=350,
              flat_ties_L16=200, flat_ties_15_16=29, inside_straddlers_listed=220)


def _floor(what, measured, floor):
    print(f"{what}: {measured} / {floor}")
    assert measured >= floor, (what, measured, floor)


def _ties(name, L):
    """-> (tie pairs, ties across 15|16, ties across 31|32) of ``name``'s lists at L."""
    tp = ref.tie_pairs(ref.select(ref.tet_intersect(name), L))
    return int(tp.sum()), int(tp[15]) if L > 16 else 0, int(tp[31]) if L > 32 else 0


def test_reach_aligned():
    old, new = ref.tet_intersect("aligned", None, False), ref.tet_intersect("aligned")
    hits, pixels = ref.edge_hits(new)
    _floor("aligned exact-edge hits", hits, FLOORS["aligned_edge_hits"])
    _floor("aligned exact-edge pixels", pixels, FLOORS["aligned_edge_pixels"])
    _floor("aligned tie pairs, L = 4", _ties("aligned", 4)[0], FLOORS["aligned_ties_L4"])
    _floor("aligned ties across 15|16, L = 17", _ties("aligned", 17)[1], FLOORS["aligned_ties_15_16"])
    _floor("aligned ties across 31|32, L = 40", _ties("aligned", 40)[2], FLOORS["aligned_ties_31_32"])
    hits, pixels = ref.rule_removed(old, new)
    _floor("aligned hits the rule removes", hits, FLOORS["aligned_removed_hits"])
    _floor("aligned pixels the rule removes a hit at", pixels, FLOORS["aligned_removed_pixels"])


@pytest.mark.parametrize("name,L", [("duplicates", 4), ("flat", 16)])
def test_reach_ties(name, L):
    _floor(f"{name} tie pairs, L = {L}", _ties(name, L)[0], FLOORS[f"{name}_ties_L{L}"])
    _floor(f"{name} ties across 15|16, L = 17", _ties(name, 17)[1], FLOORS[f"{name}_ties_15_16"])


def test_reach_long_lists():
    import tet_scenes
    th = tet_scenes.thresholds()
    chunk = ref.TILE * ref.TILE                                                     # RZ_CHUNK = TILE_PIX
    x = ref.tet_intersect("deep")
    longest = int((x["cand"] >= 0).sum(1).max())
    _floor("deep longest tile list", longest, 39 * chunk)
    _floor("deep most hits of a pixel", int(x["hit"].sum(1).max()), 33)
    assert (ref.select(x, 40)["cnt"] > 32).any()                                   # (L = 40: work in all three passes)
    x = ref.tet_intersect("deep_sort", None, True, *DEEP_SORT_SIZE)
    _floor("deep_sort longest tile list", int((x["cand"] >= 0).sum(1).max()), th["TILE_SORT_MAX"] + 1)
    for name, k in (("chunk_edge", 1), ("chunk_edge3", 3)):
        x = ref.tet_intersect(name)
        n = (x["cand"] >= 0).sum(1)
        assert (n == k * chunk + 1).all(), (name, n.min(), n.max())
        r = ref.select(x, 4)
        last = x["cand"][:, k * chunk]
        assert (r["cnt"] >= 1).all() and np.array_equal(r["layers"].reshape(-1, 4)[:, 0], last), name   # the last entry: slot 0


def test_reach_inside_straddlers():
    """``inside``: faces that straddle a view's camera plane are in tile lists (no depth bound holds for them) -- and clear
    float64 hits on such faces are missing from the lists altogether (the bbox of their mirrored projections misses the tile):
    the documented limitation, counted here."""
    s = ref.tet_case("inside")
    x = ref.tet_intersect("inside")
    st = ref.straddles(s)
    B, H, W = x["shape"]
    view = np.arange(B * H * W) // (H * W)
    in_lists = (x["cand"] >= 0) & st[view[:, None], np.where(x["cand"] >= 0, x["cand"], 0)]
    listed_faces = len(np.unique((view[:, None] * st.shape[1] + x["cand"])[in_lists]))
    _floor("inside straddling faces in some tile list", listed_faces, FLOORS["inside_straddlers_listed"])
    clear = ref.clear_hits64(s, straddlers=True)
    missing = len(ref.missing64(x, clear))
    print(f"inside: {len(clear[0])} clear float64 hits on straddling faces, {missing} of them in no list")
    assert len(clear[0]) > 0
