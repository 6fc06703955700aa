"""LayeredRenderer.render / dm2_layers_composite without a GPU: the contract's restatement (tests/layer_composite_ref.py)
against the CPU oracle's ray/triangle test and clamp, its gradients against finite differences, hand cases, and the
binding's refusals."""
import numpy as np
import pytest
import torch

import layer_composite_ref as ref
from util import ROOT, table_capacity  # noqa: F401  (ROOT: puts the repository on sys.path)

from dmesh2_renderer_amd import _C


def test_float32_pass_matches_oracle_ray_tri_and_clamp():
    """On random ray/triangle pairs (many near the edges and behind the ray) the vectorised float32 restatement gives the
    oracle's Moeller-Trumbore (t, u, v, edge case) and clamp code bit for bit."""
    from oracle import cpu as orc
    rng = np.random.RandomState(7)
    n = 3000
    ro = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    rd = rng.normal(size=(n, 3)).astype(np.float32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True).astype(np.float32)
    p = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
    p[::7, 2] = p[::7, 0] + (p[::7, 1] - p[::7, 0]) * np.float32(2.0)           # degenerate (collinear) triangles
    p[1::11, 1] = p[1::11, 0]                                                   # and coincident corners
    ok, t, u, v = ref.ray_tri32(ro, rd, p[:, 0], p[:, 1], p[:, 2])
    code = ref.clamp_code32(u, v)
    seen = set()
    for i in range(n):
        ok_o, tuv, _ = orc.ray_tri(ro[i], rd[i], p[i].reshape(-1), np.float32)
        assert ok_o == bool(ok[i]), i
        if not ok_o:
            continue
        got = np.array([t[i], u[i], v[i]], np.float32)
        assert np.array_equal(got.view(np.uint32), tuv.astype(np.float32).view(np.uint32)), (i, got, tuv)
        c, _ = orc.clamp_bary(float(u[i]), float(v[i]), np.float32)
        assert c == int(code[i]), (i, u[i], v[i])
        seen.add(c)
    assert seen == set(range(7))                                                # every region of the clamp was met
    assert (~ok).sum() > 0


def test_restatement_gradients_match_finite_differences():
    sc = ref.ortho_scene()
    sc["faces_opacity"][[1, 4]] = [1.0, 0.0]
    fwd = ref.forward32(**sc)
    assert fwd["blend"].sum() > 20 and (fwd["n_contrib"] > 1).any()
    rng = np.random.RandomState(3)
    gc = rng.normal(size=fwd["color"].shape)
    gd = rng.normal(size=fwd["depth_raw"].shape)
    g = ref.grads64(fwd, sc["faces"], sc["verts_color"], sc["faces_opacity"], sc["faces_intense"], sc["verts_ndc"],
                    sc["background"], gc, gd)
    base = {k: torch.tensor(sc[k], dtype=torch.float64) for k in ("verts_color", "faces_opacity", "faces_intense")}
    base["verts_ndc_z"] = torch.tensor(sc["verts_ndc"][..., 2], dtype=torch.float64)

    def loss(vals):
        c, d = ref.composite64(fwd, sc["faces"], vals["verts_color"], vals["faces_opacity"], vals["faces_intense"],
                               vals["verts_ndc_z"], sc["background"].astype(np.float64))
        return float((c.numpy() * gc).sum() + (d.numpy() * gd).sum())

    eps = 1e-6
    for name, key in (("verts_color", "verts_color"), ("faces_opacity", "faces_opacity"), ("faces_intense", "faces_intense"),
                      ("verts_ndc_z", "verts_ndc")):
        analytic = g[key][..., 2] if name == "verts_ndc_z" else g[key]
        flat = analytic.reshape(-1)
        idx = np.argsort(-np.abs(flat))[:6].tolist() + rng.randint(0, flat.size, 4).tolist()
        for i in idx:
            hi = {k: v.clone() for k, v in base.items()}; lo = {k: v.clone() for k, v in base.items()}
            hi[name].view(-1)[i] += eps; lo[name].view(-1)[i] -= eps
            fd = (loss(hi) - loss(lo)) / (2 * eps)
            assert abs(fd - flat[i]) <= 1e-6 * max(1.0, abs(fd)), (name, i, fd, flat[i])
    assert np.abs(g["faces_opacity"]).max() > 0 and np.abs(g["verts_ndc"][..., :2]).max() == 0


def test_empty_layers_give_the_background():
    sc = ref.ortho_scene(L=3)
    sc["render_layers"][:] = -1
    fwd = ref.forward32(**sc)
    assert np.array_equal(fwd["color"], np.broadcast_to(sc["background"], fwd["color"].shape))
    assert np.all(fwd["depth_raw"] == 1.0) and np.all(fwd["final_T"] == 1.0) and np.all(fwd["n_contrib"] == 0)
    assert np.all(1.0 - (fwd["depth_raw"] + 1.0) / 2.0 == 0.0)                  # the module's depth: 0 = background
    fwd0 = ref.forward32(**dict(sc, render_layers=np.zeros(sc["render_layers"].shape[:3] + (0,), np.int32)))
    assert np.array_equal(fwd0["color"], fwd["color"]) and np.all(fwd0["n_contrib"] == 0)


def test_one_opaque_face_gives_its_interpolated_colour():
    """One face of opacity 1 over the whole frame: each pixel shows the barycentric mix of the vertex colours (times the
    intensity), the depth is the mix of the z values, the background is gone."""
    sc = ref.ortho_scene(B=1, H=5, W=6, L=1, F=1, holes=False)
    sc["verts"][:3] = [[-1.0, -1.0, -2.0], [3.0, -1.0, -2.0], [-1.0, 3.0, -2.0]]
    sc["faces_opacity"][:] = 1.0
    sc["render_layers"][:] = 0
    fwd = ref.forward32(**sc)
    assert np.all(fwd["n_contrib"] == 1) and np.all(fwd["final_T"] == 0.0)
    ro = sc["ray_o"][0].astype(np.float64)
    u = (ro[..., 0] + 1) / 4; v = (ro[..., 1] + 1) / 4                       # barycentrics of the pixel centre
    w = np.stack([1 - u - v, u, v], -1)
    want = (w @ sc["verts_color"][:3].astype(np.float64)) * sc["faces_intense"][0, 0]
    assert np.allclose(fwd["color"][0], want, atol=1e-6)
    assert np.allclose(fwd["depth_raw"][0], w @ sc["verts_ndc"][0, :3, 2].astype(np.float64), atol=1e-6)


def test_opacity_one_ends_the_list():
    sc = ref.ortho_scene(B=1, L=4, holes=False)
    fwd_all = ref.forward32(**sc)
    sc["faces_opacity"][:] = 1.0
    fwd = ref.forward32(**sc)
    hit_any = fwd_all["blend"].any(-1)
    # the first layer that blends ends the list: exactly one blend per pixel that has any, T = 0 behind it
    assert np.array_equal(fwd["blend"].sum(-1), hit_any.astype(np.int64))
    assert np.all(fwd["final_T"][hit_any] == 0.0)
    first = np.argmax(fwd_all["blend"], -1)
    assert np.array_equal(fwd["n_contrib"][hit_any], first[hit_any] + 1)
    # and its gradients are finite (the backward divides by nothing)
    g = ref.grads64(fwd, sc["faces"], sc["verts_color"], sc["faces_opacity"], sc["faces_intense"], sc["verts_ndc"],
                    sc["background"], np.ones(fwd["color"].shape), np.ones(fwd["depth_raw"].shape))
    assert all(np.isfinite(v).all() for v in g.values()) and np.abs(g["faces_opacity"]).max() > 0


def test_default_ortho_scene_is_not_crowded():
    """``crowded`` off leaves the scene as it was: same arrays as the crowded one but for the triangles' xy."""
    a, b = ref.ortho_scene(seed=3, holes=False), ref.ortho_scene(seed=3, holes=False, crowded=True)
    for k in a:
        if k != "verts":
            assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["verts"][:, 2], b["verts"][:, 2])
    ta, tb = a["verts"].reshape(-1, 3, 3)[:, :, :2], b["verts"].reshape(-1, 3, 3)[:, :, :2]
    assert np.allclose(tb - tb.mean(1, keepdims=True), 5 * (ta - ta.mean(1, keepdims=True)), atol=1e-5)
    assert ref.forward32(**b)["blend"].mean() > 0.99 > ref.forward32(**a)["blend"].mean()


@pytest.mark.parametrize("name", list(ref.CROWDED))
def test_crowded_cases_against_the_face_table(name):
    """The scenes the GPU tests use for the face table's overflow route (dm2_face_table.h: lc_slot returns -1) hold what
    those tests rely on, against the LC_SLOTS the header has today: every 16 x 16 tile blends more distinct faces than the
    table has slots (overflow), or at most that many and more than 0.8 of them (nearly full).  And on them the float32 pass
    is the float64 one: per pixel the blend weights alpha * T sum to at most 1 and a layer's term (colour * intensity <= 1.5,
    |z| <= 1) carries about 9 roundings of its own, 2 per layer in front of it through T and one of the running sum, hence
    1.5 * (3 L + 12) units of 2^-24."""
    sc, kind = ref.crowded_case(name)
    L, F = sc["render_layers"].shape[-1], sc["faces"].shape[0]
    fwd = ref.forward32(**sc)
    lo, hi = ref.distinct_blended_per_tile(fwd)
    print(f"{name}: F = {F}, L = {L}, {fwd['blend'].mean():.4f} of the slots blend, {lo}..{hi} distinct blended faces per tile, "
          f"table of {table_capacity()}")
    ref.check_crowded(kind, lo, hi, table_capacity())
    assert kind in ("overflow", "nearly_full")
    # the edits are met: opacity-1 faces ended lists, opacity-0 faces blended, a face blended twice in a pixel
    f_bl = np.where(fwd["blend"], fwd["fs"], -1)
    assert (fwd["final_T"] == 0.0).sum() > 100 and (sc["faces_opacity"][f_bl[f_bl >= 0]] == 0.0).sum() > 100
    assert ((f_bl[..., 0] == f_bl[..., 1]) & (f_bl[..., 0] >= 0)).sum() > 100
    t64 = lambda k: torch.tensor(sc[k], dtype=torch.float64)
    c, d = ref.composite64(fwd, sc["faces"], t64("verts_color"), t64("faces_opacity"), t64("faces_intense"),
                           t64("verts_ndc")[..., 2], sc["background"])
    bound = 1.5 * (3 * L + 12) * 2.0 ** -24
    assert np.abs(c.numpy() - fwd["color"]).max() <= bound and np.abs(d.numpy() - fwd["depth_raw"]).max() <= bound


def test_composite_layers_cuda_refuses_cpu_tensors():
    sc = ref.ortho_scene(B=1)
    t = {k: torch.from_numpy(v) for k, v in sc.items()}
    args = (t["render_layers"], t["verts"], t["faces"], t["verts_color"], t["faces_opacity"], t["faces_intense"], t["verts_ndc"],
            t["background"], t["ray_o"], t["ray_d"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.composite_layers_cuda(*args)
    B, H, W = t["render_layers"].shape[:3]
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.composite_layers_backward_cuda(*args, torch.zeros((B, H, W), dtype=torch.int32), torch.zeros((B, H, W, 3)),
                                          torch.zeros((B, H, W)))


def test_layered_renderer_render_refuses_cpu_tensors():
    import dmesh2_renderer_amd as dm2
    from dmesh2_renderer_amd import scenes
    ts = scenes.tet_lattice(32, 24, 2, seed=scenes.SEED_BASE + 3)
    lr = dm2.LayeredRenderer(ts.mv, ts.proj, 32, 24, "cpu", fused_prep=False)
    P, F = ts.verts.shape[0], ts.faces.shape[0]
    layers = torch.full((1, 24, 32, 2), -1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lr.render([0], layers, ts.verts, ts.faces, torch.rand(P, 3), torch.rand(F), torch.rand(1, F), torch.zeros(3))


def test_composite_desc_matches_header_layout():
    """The ctypes mirror of dm2_layer_composite_desc: field order, sizes and offsets as the C compiler lays them out."""
    import ctypes
    from test_cabi import header_struct
    decl = header_struct("dm2_layer_composite_desc")
    cls = _C.LayerCompositeDesc
    assert [f[0] for f in decl] == [f[0] for f in cls._fields_]
    off = 0
    for (nm, size, is_ptr), (cnm, ctype) in zip(decl, cls._fields_):
        off = (off + size - 1) // size * size
        cf = getattr(cls, cnm)
        assert (cf.offset, cf.size) == (off, size), nm
        assert (ctype is ctypes.c_void_p) == is_ptr, nm
        off += size
    assert ctypes.sizeof(cls) == (off + 7) // 8 * 8
