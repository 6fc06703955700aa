"""The restatement of Renderer.coverage's contract (tests/coverage_ref.py) against the reference's own numbers, against central
differences of the float64 area, and the point of the op: a silhouette loss through coverage * opacity moves the projected
vertices, through the per-face opacity alone it does not.  No GPU."""
import numpy as np
import pytest

import composite_ref
import coverage_ref as ref
from util import table_capacity

f32 = np.float32


@pytest.mark.parametrize("name,key", ref.FIXTURE_CASES)
def test_fixture_cases_reproduce_the_reference_areas(name, key):
    """At temperature 1 cov is the area itself: within the 2e-6 of test_gpu_clippers.py of the reference's analytic area, and 0
    exactly where the reference raises.  The ids outside [0, F) and the faces with a vertex outside the table give 0."""
    c = ref.fixture_case(name, key)
    i = c["info"][1.0]
    y, x, l = c["slot"].T
    cov = i["cov"][0, y, x, l]
    raised = np.array([bool(m) for m in c["golden"]["msg_analytic"]])
    assert np.array_equal(i["error"][0, y, x, l], raised)
    assert not cov[raised].any()
    assert np.abs(cov[~raised] - c["golden"]["area_analytic"][~raised]).max() <= 2e-6
    listed = np.zeros(c["render_layers"].shape, bool)
    listed[0, y, x, l] = True
    rest = c["render_layers"][~listed]
    assert (rest != -1).sum() >= 6 and i["empty"][~listed].all() and not i["cov"][~listed].any()
    # the other temperatures: the mix of the same areas; 0 stays 0 (an empty slot, an error, a zero area), a hit at temperature 0 is 1
    half = c["info"][0.5]["cov"][0, y, x, l]
    ok = ~raised & (i["area"][0, y, x, l] != 0)
    assert np.array_equal(half[ok], (np.float64(f32(0.5)) + (i["area"][0, y, x, l][ok] * f32(0.5)).astype(np.float64)).astype(f32))
    assert not half[~ok].any()
    zero_t = c["info"][0.0]
    assert np.array_equal(zero_t["cov"], np.where(i["empty"], f32(0), f32(1))) and not zero_t["J"].any()


def _general_position(tri, pixmin, margin):
    """No triangle corner within ``margin`` of a pixel boundary line, no pixel corner within ``margin`` of an edge's line, no edge
    component below 0.05: the clipped polygon keeps its shape under a perturbation well below ``margin``."""
    tri = np.asarray(tri, np.float64)
    lines = np.array([pixmin[0], pixmin[0] + 1.0, pixmin[1], pixmin[1] + 1.0])
    if np.abs(tri[:, 0, None] - lines[None, :2]).min() < margin or np.abs(tri[:, 1, None] - lines[None, 2:]).min() < margin:
        return False
    corners = np.array([[lines[0], lines[2]], [lines[1], lines[2]], [lines[1], lines[3]], [lines[0], lines[3]]])
    for k in range(3):
        p, e = tri[k], tri[(k + 1) % 3] - tri[k]
        if np.abs(e).min() < 0.05:
            return False
        d = np.abs((corners[:, 0] - p[0]) * e[1] - (corners[:, 1] - p[1]) * e[0]) / np.hypot(*e)
        if d.min() < margin:
            return False
    return True


@pytest.mark.parametrize("which", ["aa_pairs", "overflow"])
def test_gradient_against_central_differences(which):
    """grad_image64 (float32 Jacobians of the oracle, times g_cov * temperature, through the undone reorder) against central
    differences of the float64 area over every coordinate of the partial slots' vertices, temperature 0.5, on the slots in
    general position (each face is listed once and owns its vertices, so a coordinate moves one slot).

    Tolerance 1e-4 of max(1, |g|): the float32 clipper rounds its crossing coordinates to half an ulp of a coordinate < 64, 1.9e-6,
    and a Jacobian entry is a product of such coordinates' differences with t and the factor 1/e of a crossing (aa.h:276-294),
    |e| >= 0.05 here: 20 x 1.9e-6 = 4e-5 per crossing, two crossings per corner at most.  The central difference itself (h = 1e-5 on
    a piecewise rational function with |e| >= 0.05, float64) is good to 1e-8."""
    c = ref.fixture_case("aa_pairs", "tri_in") if which == "aa_pairs" else ref.overflow_case()
    T, h = 0.5, 1e-5
    info = c["info"][T]
    got = ref.grad_image64(c["render_layers"], c["verts_image"], c["faces"], T, c["g"], info)
    vi = c["verts_image"].astype(np.float64)
    checked, worst = 0, 0.0
    for b, y, x, l in np.argwhere(info["partial"]).tolist()[:200]:
        f = int(c["render_layers"][b, y, x, l])
        g = float(c["g"][b, y, x, l])
        tri = vi[b, c["faces"][f]]
        if g == 0 or not _general_position(tri, (x, y), 1e-3):
            continue
        for k in range(3):
            v = int(c["faces"][f, k])
            for a in range(2):
                ap, am = tri.copy(), tri.copy()
                ap[k, a] += h
                am[k, a] -= h
                (Ap, cp), (Am, cm) = ref.area64(ap, (x, y)), ref.area64(am, (x, y))
                assert cp == 0 and cm == 0
                fd = g * T * (Ap - Am) / (2 * h)
                worst = max(worst, abs(got[b, v, a] - fd) / max(1.0, abs(g)))
                assert abs(got[b, v, a] - fd) <= 1e-4 * max(1.0, abs(g)), (b, y, x, l, k, a, got[b, v, a], fd)
        checked += 1
    print(which, "slots checked", checked, "worst", worst)
    assert checked >= (60 if which == "aa_pairs" else 100)         # of the 137 / the first 200 partial slots
    # and where nothing flows: vertices of faces that are not listed partial get exactly nothing
    part_faces = c["render_layers"][info["partial"]]
    used = np.zeros(vi.shape[1], bool)
    used[c["faces"][part_faces].reshape(-1)] = True
    assert not got[0, ~used].any() and got[0, used].any()


def test_upstream_zero_and_temperature_zero_give_no_gradient():
    c = ref.overflow_case()
    assert not ref.grad_image64(c["render_layers"], c["verts_image"], c["faces"], 1.0, np.zeros_like(c["g"]), c["info"][1.0]).any()
    assert not ref.grad_image64(c["render_layers"], c["verts_image"], c["faces"], 0.0, c["g"], c["info"][0.0]).any()
    with pytest.raises(ValueError):
        ref.coverage32(c["render_layers"], c["verts_image"], c["faces"], 1.5)


def test_a_silhouette_loss_moves_the_triangle_only_through_coverage():
    """One opaque triangle on a background, loss = acc.sum() of composite: with alpha = opacity * cov the gradient w.r.t. the
    projected vertices is non-zero and agrees with moving the triangle; with the per-face opacity alone acc does not depend on
    them at all."""
    H = W = 12
    vi = np.array([[[2.3, 1.7], [9.6, 3.2], [4.4, 10.1]]], f32)
    faces = np.array([[0, 1, 2]], np.int32)
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    a, b, c = vi[0].astype(np.float64)
    side = lambda p, q: (q[0] - p[0]) * (ys - p[1]) - (q[1] - p[1]) * (xs - p[0])
    s0, s1, s2 = side(a, b), side(b, c), side(c, a)
    inside = ((s0 >= 0) & (s1 >= 0) & (s2 >= 0)) | ((s0 <= 0) & (s1 <= 0) & (s2 <= 0))
    rl = np.where(inside, 0, -1).astype(np.int32)[None, ..., None]                  # the pixels whose centre the triangle covers
    assert 20 < inside.sum() < 60
    opacity = np.array([1.0], f32)
    values = np.ones((1, H, W, 1, 3), f32)
    bg = np.zeros(3, f32)

    def acc_sum(v, with_cov):
        alpha = opacity[np.where(rl >= 0, rl, 0)] * (ref.coverage32(rl, v, faces, 1.0)["cov"] if with_cov else f32(1))
        T = composite_ref.forward32(values, alpha.astype(f32), rl, bg)[1]
        return float((1.0 - T.astype(np.float64)).sum())

    info = ref.coverage32(rl, vi, faces, 1.0)
    assert info["partial"].sum() >= 8 and info["full"].sum() >= 8
    alpha = (opacity[np.where(rl >= 0, rl, 0)] * info["cov"]).astype(f32)
    n = composite_ref.forward32(values, alpha, rl, bg)[2]
    _, dalpha = composite_ref.grads64(values, alpha, rl, bg, n, None, np.ones((1, H, W)))
    g_cov = dalpha * opacity[np.where(rl >= 0, rl, 0)]
    gi = ref.grad_image64(rl, vi, faces, 1.0, g_cov, info)
    assert np.abs(gi).max() > 0.1
    step = f32(1.0 / 64)                                                              # exact in float32 at these coordinates
    for k in range(3):
        for ax in range(2):
            vp, vm = vi.copy(), vi.copy()
            vp[0, k, ax] += step
            vm[0, k, ax] -= step
            fd = (acc_sum(vp, True) - acc_sum(vm, True)) / (2 * float(step))
            assert abs(gi[0, k, ax] - fd) <= 0.02 * max(1.0, abs(fd)), (k, ax, gi[0, k, ax], fd)   # (second order in a 1/64 step)
            assert acc_sum(vp, False) == acc_sum(vm, False) == acc_sum(vi, False)     # piecewise constant: gradient exactly zero


def test_cases_are_not_hollow():
    cap = table_capacity()
    for name, L in ref.SCENE_CASES:
        c = ref.scene_case(name, L)
        i = c["info"][1.0]
        if name == "no_faces":
            assert c["faces"].shape[0] == 0 and i["empty"].all()
            continue
        assert i["partial"].sum() >= 1000, (name, L)
        m = ~i["empty"]
        sw = ref.swapped(c["verts_image"], c["faces"])[np.argwhere(m)[:, 0], c["render_layers"][m]]
        assert sw.any() and (~sw).any(), (name, L)
        assert c["W"] % 16 or c["H"] % 16                                    # partial tiles
    n_err = sum(int(ref.fixture_case(n, "tri_in")["info"][1.0]["error"].sum()) for n in ("aa_pairs", "aa_error_pairs"))
    n_zero = sum(int(ref.fixture_case(n, "tri_in")["info"][1.0]["zero"].sum()) for n in ("aa_pairs", "aa_error_pairs"))
    assert n_err >= 10 and n_zero >= 20
    for n, k in ref.FIXTURE_CASES:
        i = ref.fixture_case(n, k)["info"][1.0]
        assert i["error"].any() and i["zero"].any() and i["full"].any() and i["partial"].any()
    o = ref.overflow_case()
    assert o["render_layers"].shape[1:3] == (16, 16)
    part = np.unique(o["render_layers"][o["info"][1.0]["partial"]])
    assert len(part) > cap and len(np.unique(o["render_layers"])) == o["render_layers"].size
    sw = ref.swapped(o["verts_image"], o["faces"])[0]
    assert sw.sum() > cap // 4 and (~sw).sum() > cap // 4
    assert (o["g"] == 0).sum() > 20
