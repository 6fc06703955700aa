"""The front end's call contract, without a GPU: what ``Renderer`` / ``LayeredRenderer`` and the autograd Functions hand to
``_C`` (tests/frontend_trace.py) for every public method -- ray tensors and analytic rays, full frame, an unaligned window and
an empty one, with and without alpha and face weights, forward and backward, the side channels seen inside each call.

The expected records (tests/golden/frontend_calls.json) were taken before the front end's three decisions -- which rays, how
``verts`` is projected, window or full frame -- were each written once, so a full-frame body and a window body cannot drift
apart unseen.  Regenerate with ``python tests/golden/make_golden.py --only-frontend-calls`` only when the contract is meant to
change.

Pinned as it stands: ``forward`` has no early-out for an empty patch (``test_forward_has_no_early_out_for_an_empty_patch`` and the
``forward-empty-*`` records); ``render`` without ``patch_min`` checks no rank and
``coverage`` without ``patch_min`` no frame size (the op does); ``generate`` is driven with ``verts`` that do not require grad
(its projection is a constant of the op either way).
"""
import json
import os
import re

import pytest
import torch

import frontend_trace as ft
from frontend_trace import CAMS, H, L, W, Scene, layers_of, recording, window_args

import dmesh2_renderer_amd as dm

i32, f32 = torch.int32, torch.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "frontend_calls.json")) as f:
        return json.load(f)


def test_cases_are_the_golden_ones(golden):
    assert sorted(golden) == sorted(ft.CASES)


@pytest.mark.parametrize("name", sorted(ft.CASES))
def test_calls_equal_the_recorded_ones(golden, name):
    got = json.loads(json.dumps(ft.describe_calls(ft.run_case(name))))          # (tuples -> lists, as the file holds them)
    want = golden[name]
    assert [c["entry"] for c in got] == [c["entry"] for c in want]
    for g, w in zip(got, want):
        assert g == w, g["entry"]
    if "-empty-" in name and not name.startswith("forward-"):
        assert got == []                                    # an empty window launches nothing


@pytest.mark.parametrize("name", sorted(n for n in ft.CASES if n.startswith("forward-empty-")))
def test_forward_has_no_early_out_for_an_empty_patch(name):
    """Pinned as it stands: ``forward`` hands a 0-wide patch to the op like any other (exactly one forward call, its backwards
    behind it), where the deferred ops return empty tensors and call nothing."""
    calls = ft.run_case(name)
    fwd = [c for c in calls if c.entry == "render_forward_cuda"]
    assert len(fwd) == 1 and calls[0] is fwd[0] and all(c.entry == "render_backward_cuda" for c in calls[1:])
    assert (fwd[0].args["patch_width"], fwd[0].args["patch_height"]) == ft.WINDOWS["empty"][1:] == (0, 7)
    assert fwd[0].args["patch_min"].tolist() == ft.WINDOWS["empty"][0] and fwd[0].channels["window"] is None
    analytic = "-ana1-" in name
    assert tuple(fwd[0].args["image_ray_o"].shape) == ((2, 0, 0, 3) if analytic else (2, 7, 0, 3))
    assert (fwd[0].channels["analytic"] is not None) == analytic


# -- what the records cannot hold: values and identities ----------------------------------------------------------------------
def _drive(method, analytic, win, s=None, cams=CAMS):
    """One forward of ``method`` -> (renderer, scene, the calls)."""
    s = s or Scene()
    layered = method in ("generate", "render")
    r = s.renderer(analytic, layered=layered)
    rl = layers_of(win, cams)
    with recording() as calls:
        if method == "forward":
            pm, pw, ph = ([[0, 0], [0, 0]], W, H) if ft.WINDOWS[win] is None else ft.WINDOWS[win]
            r(cams, torch.tensor(pm, dtype=i32), pw, ph, s.verts, s.faces, s.verts_color, s.faces_opacity, s.faces_intense, s.background)
        elif method == "rasterize":
            r.rasterize(cams, s.verts, s.faces, L, **window_args(win))
        elif method == "generate":
            r.generate(cams, s.verts, s.faces, s.tets, s.face_tets, s.tet_faces, s.faces_existence, L, **window_args(win))
        elif method == "render":
            r.render(cams, rl, s.verts, s.faces, s.verts_color, s.faces_opacity, s.faces_intense, s.background,
                     **window_args(win, sized=False))
        elif method == "shading_vectors":
            r.shading_vectors(cams, rl, torch.ones(tuple(rl.shape)), **window_args(win, sized=False))
        elif method == "coverage":
            r.coverage(cams, rl, s.verts, s.faces, **window_args(win, sized=False))
        elif method == "bary_derivatives":
            r.bary_derivatives(cams, rl, s.verts, s.faces, **window_args(win, sized=False))
    return r, s, calls


RAY_METHODS = ("forward", "rasterize", "generate", "render", "shading_vectors")
WINDOW_METHODS = ("rasterize", "generate", "render", "shading_vectors", "coverage", "bary_derivatives")


@pytest.mark.parametrize("method", RAY_METHODS)
def test_full_frame_rays_of_consecutive_cameras_are_views(method):
    r, _, calls = _drive(method, False, "full")
    (c,) = calls
    for got, frame in ((c.args["image_ray_o"], r.ray_o), (c.args["image_ray_d"], r.ray_d)):
        assert got.untyped_storage().data_ptr() == frame.untyped_storage().data_ptr()      # no copy
        assert got.storage_offset() == frame[CAMS[0]].storage_offset() and tuple(got.shape) == (len(CAMS), H, W, 3)
        assert torch.equal(got, frame[CAMS])


@pytest.mark.parametrize("method", RAY_METHODS)
@pytest.mark.parametrize("cams", [CAMS, [2, 0]])
def test_window_rays_are_the_frames_slice_at_patch_min(method, cams):
    r, _, calls = _drive(method, False, "window", cams=cams)
    (c,) = calls
    pm, pw, ph = ft.WINDOWS["window"]
    for got, frame in ((c.args["image_ray_o"], r.ray_o), (c.args["image_ray_d"], r.ray_d)):
        want = torch.stack([frame[cam, y:y + ph, x:x + pw] for cam, (x, y) in zip(cams, pm)])
        assert got.dtype == f32 and torch.equal(got, want)


@pytest.mark.parametrize("method", RAY_METHODS)
@pytest.mark.parametrize("win", ["full", "window"])
@pytest.mark.parametrize("cams", [CAMS, [2, 0]])
def test_analytic_rays_carry_the_selected_cameras(method, win, cams):
    r, _, calls = _drive(method, True, win, cams=cams)
    (c,) = calls
    cam, w, h = c.channels["analytic"]
    assert torch.equal(cam, r.ray_cam[cams]) and cam.is_contiguous() and (w, h) == (W, H)
    assert r.ray_o is None and tuple(c.args["image_ray_o"].shape) == (len(cams), 0, 0, 3)
    assert c.args["image_ray_o"].dtype == f32 and tuple(c.args["image_ray_d"].shape) == (len(cams), 0, 0, 3)


@pytest.mark.parametrize("analytic", [False, True])
def test_bary_derivatives_cameras_are_the_analytic_rows(analytic):
    r, s, calls = _drive("bary_derivatives", analytic, "full")
    want = torch.cat((torch.inverse(s.mv[CAMS]).reshape(-1, 16), torch.inverse(s.proj[CAMS]).reshape(-1, 16)), dim=1)
    assert torch.equal(calls[0].args["ray_cam"], want) and calls[0].args["ray_cam"].is_contiguous()
    if analytic:
        assert torch.equal(calls[0].args["ray_cam"], r.ray_cam[CAMS])


@pytest.mark.parametrize("method", WINDOW_METHODS)
@pytest.mark.parametrize("analytic", [False, True])
def test_window_channel_carries_the_callers_patch_min(method, analytic):
    _, _, calls = _drive(method, analytic, "window")
    pm, fw, fh = calls[0].channels["window"]
    assert pm.dtype == i32 and pm.tolist() == ft.WINDOWS["window"][0] and (fw, fh) == (W, H)
    _, _, calls = _drive(method, analytic, "full")
    assert calls[0].channels["window"] is None


@pytest.mark.parametrize("analytic", [False, True])
def test_forward_hands_patch_min_to_the_op_not_to_the_window_channel(analytic):
    _, _, calls = _drive("forward", analytic, "window")
    assert calls[0].channels["window"] is None and calls[0].args["patch_min"].tolist() == ft.WINDOWS["window"][0]
    assert (calls[0].args["patch_width"], calls[0].args["patch_height"]) == ft.WINDOWS["window"][1:]


@pytest.mark.parametrize("method,win,graph", [
    ("rasterize", "full", False), ("rasterize", "window", False), ("generate", "window", False),
    ("coverage", "full", True), ("coverage", "window", True), ("render", "full", True), ("render", "window", True),
    ("forward", "full", True), ("forward", "window", True)])
def test_projection_carries_a_graph_only_where_the_op_differentiates_it(method, win, graph, monkeypatch):
    """rasterize and generate take the projection as constants; coverage, render and forward differentiate through it."""
    seen = []
    real = dm.Renderer.compute_verts_ndc_image

    def spy(self, verts, mv, proj):
        out = real(self, verts, mv, proj)
        seen.append(out)
        return out
    monkeypatch.setattr(dm.Renderer, "compute_verts_ndc_image", spy)
    _, s, _ = _drive(method, False, win)
    assert s.verts.requires_grad and len(seen) == 1
    assert [t.requires_grad for t in seen[0]] == [graph, graph]
    seen.clear()
    _drive(method, False, win, s=Scene(grad=False))
    assert [t.requires_grad for t in seen[0]] == [False, False]


def test_backward_sees_the_forwards_channels_not_the_ambient_ones():
    """A window call's backward, run outside every block, and inside a foreign one: it sees what its forward saw."""
    s = Scene()
    r = s.renderer(True)
    with recording() as calls:
        out = r.rasterize(CAMS, s.verts, s.faces, L, **window_args("window"))
        foreign = torch.zeros((2, 2), dtype=i32)
        with dm._C.window(foreign, 5, 5), dm._C.analytic_rays(None, 0, 0):
            out[2].sum().backward()
    fwd, bwd = calls
    assert bwd.entry == "rasterize_layers_backward_cuda"
    assert bwd.channels["window"][0] is fwd.channels["window"][0] and bwd.channels["window"][1:] == (W, H)
    assert bwd.channels["analytic"][0] is fwd.channels["analytic"][0]
    s = Scene()
    with recording() as calls:
        out = s.renderer(False).rasterize(CAMS, s.verts, s.faces, L)
        with dm._C.window(torch.zeros((2, 2), dtype=i32), 5, 5), dm._C.analytic_rays(torch.zeros((2, 32)), 5, 5):
            out[2].sum().backward()
    assert calls[1].channels["window"] is None and calls[1].channels["analytic"] is None      # None channels are entered as off


# -- the bad calls: type, message and which error wins -----------------------------------------------------------------------
PAIR_SIZE = "patch_width / patch_height need patch_min"
PAIR_MIN = "patch_min needs patch_width and patch_height"
RANK = "render_layers must have dimensions (B, H, W, L), got (2, 7, 9)"
NEGATIVE = "patch_min must not be negative"
PAST_X, PAST_Y = "Some b_patch_max_x exceed self.width", "Some b_patch_max_y exceed self.height"


def _pm(rows=((3, 5), (7, 2))):
    return torch.tensor(rows, dtype=i32)


def _call(method, **kw):
    """``method`` of a fresh renderer with the window case's other arguments and ``kw`` in place of the window's."""
    s = Scene()
    r = s.renderer(False, layered=method in ("generate", "render"))
    rl = kw.pop("render_layers", layers_of("window"))
    if method == "rasterize":
        return r.rasterize(CAMS, s.verts, s.faces, L, **kw)
    if method == "generate":
        return r.generate(CAMS, s.verts, s.faces, s.tets, s.face_tets, s.tet_faces, s.faces_existence, L, **kw)
    if method == "render":
        return r.render(CAMS, rl, s.verts, s.faces, s.verts_color, s.faces_opacity, s.faces_intense, s.background, **kw)
    if method == "coverage":
        return r.coverage(CAMS, rl, s.verts, s.faces, **kw)
    if method == "bary_derivatives":
        return r.bary_derivatives(CAMS, rl, s.verts, s.faces, **kw)
    if method == "shading_vectors":
        return r.shading_vectors(CAMS, rl, torch.ones(tuple(rl.shape)), **kw)
    raise KeyError(method)


def _rejects(exc, message, method, **kw):
    with recording() as calls, pytest.raises(exc, match="^" + re.escape(message) + "$"):
        _call(method, **kw)
    assert calls == []


@pytest.mark.parametrize("method", ["rasterize", "generate"])
def test_sized_window_errors(method):
    _rejects(ValueError, PAIR_SIZE, method, patch_width=9)
    _rejects(ValueError, PAIR_SIZE, method, patch_height=7)
    _rejects(ValueError, PAIR_MIN, method, patch_min=_pm())
    _rejects(ValueError, PAIR_MIN, method, patch_min=_pm(), patch_width=9)
    _rejects(ValueError, PAIR_MIN, method, patch_min=_pm(((-1, 0), (0, 0))), patch_height=7)               # pairing first
    _rejects(ValueError, "patch_min must have dimensions (2, 2), got (1, 2)", method, patch_min=_pm(((3, 5),)), patch_width=9, patch_height=7)
    _rejects(ValueError, "patch_min must have dimensions (2, 2), got (4,)", method, patch_min=torch.zeros(4, dtype=i32), patch_width=-1,
             patch_height=7)                                                                                # shape before size
    _rejects(ValueError, "patch_width and patch_height must not be negative", method, patch_min=_pm(((-1, 0), (0, 0))), patch_width=-1,
             patch_height=7)                                                                                # size before origin
    _rejects(ValueError, NEGATIVE, method, patch_min=_pm(((3, -1), (30, 2))), patch_width=9, patch_height=7)   # origin before frame
    _rejects(AssertionError, PAST_X, method, patch_min=_pm(((3, 5), (12, 12))), patch_width=9, patch_height=7)  # x before y
    _rejects(AssertionError, PAST_Y, method, patch_min=_pm(((3, 5), (7, 12))), patch_width=9, patch_height=7)
    _rejects(AssertionError, PAST_X, method, patch_min=_pm(((3, 5), (21, 2))), patch_width=0, patch_height=7)   # empty windows are checked too


@pytest.mark.parametrize("method", ["render", "coverage", "bary_derivatives", "shading_vectors"])
def test_layer_window_errors(method):
    _rejects(ValueError, RANK, method, render_layers=torch.zeros((2, 7, 9), dtype=i32), patch_min=_pm())
    _rejects(ValueError, "patch_min must have dimensions (2, 2), got (2, 3)", method, patch_min=torch.zeros((2, 3), dtype=i32))
    _rejects(ValueError, NEGATIVE, method, patch_min=_pm(((3, 5), (-7, 2))))
    _rejects(AssertionError, PAST_X, method, patch_min=_pm(((3, 5), (12, 2))))
    _rejects(AssertionError, PAST_Y, method, patch_min=_pm(((3, 12), (7, 2))))
    _rejects(AssertionError, PAST_X, method, render_layers=torch.zeros((2, 7, 0, L), dtype=i32), patch_min=_pm(((3, 5), (21, 2))))


@pytest.mark.parametrize("method", ["bary_derivatives", "shading_vectors"])
def test_full_frame_rank_and_size_errors(method):
    _rejects(ValueError, RANK, method, render_layers=torch.zeros((2, 7, 9), dtype=i32))
    _rejects(ValueError, "render_layers must cover the 20 x 18 frame (or come with patch_min), got (2, 7, 9, 2)", method)


@pytest.mark.parametrize("method", ["render", "coverage"])
def test_full_frame_render_and_coverage_leave_rank_and_size_to_the_op(method):
    with recording() as calls:
        _call(method)                                       # a (2, 7, 9, 2) render_layers without patch_min: handed over as it is
    assert tuple(calls[0].args["render_layers"].shape) == (2, 7, 9, L)


def test_coverage_errors():
    rl = layers_of("window")
    _rejects(ValueError, "temperature must be in the range [0, 1]", "coverage", temperature=1.5, inside=torch.zeros(3), patch_min=_pm())
    _rejects(ValueError, "temperature must be in the range [0, 1]", "coverage", temperature=-0.1)
    _rejects(ValueError, "inside must have dimensions (2, 7, 9), got (3,)", "coverage", render_layers=rl[..., 0], inside=torch.zeros(3),
             patch_min=_pm())                                                                               # inside before rank
    _rejects(ValueError, "inside must have dimensions (2, 7, 9, 2), got (2, 7, 9)", "coverage", inside=rl[..., 0])


def test_forward_errors():
    s = Scene()
    args = (s.verts, s.faces, s.verts_color, s.faces_opacity, s.faces_intense, s.background)
    with recording() as calls:
        with pytest.raises(AssertionError, match="^" + re.escape(PAST_X) + "$"):
            s.renderer(False)(CAMS, _pm(((3, 5), (12, 12))), 9, 7, *args)
        with pytest.raises(AssertionError, match="^" + re.escape(PAST_Y) + "$"):
            s.renderer(False)(CAMS, _pm(((3, 5), (7, 12))), 9, 7, *args)
        with pytest.raises(TypeError, match="^RenderFunction takes 21 inputs, got 3$"):
            dm.RenderFunction.apply(s.verts, s.faces, 1)
    assert calls == []
    with recording() as calls:                              # analytic rays: no ray tensors to cut, so no bound check here
        s.renderer(True)(CAMS, _pm(((3, 5), (12, 12))), 9, 7, *args)
    assert len(calls) == 1


def test_standard_rasterize_calls_take_no_keyword(monkeypatch):
    """The standard mode's forward and backward are the positional calls they were before overlap mode existed (the GPU tests'
    spies take positional arguments only); overlap mode adds ``overlap=True`` to both."""
    seen = []
    monkeypatch.setattr(dm._C, "rasterize_layers_cuda", lambda *a, **kw: seen.append(kw) or ft.FAKES["rasterize_layers_cuda"](
        dict(verts_ndc=a[5], height=a[1], width=a[0], num_layers=a[9], overlap=kw.get("overlap", False))))
    monkeypatch.setattr(dm._C, "rasterize_layers_backward_cuda", lambda *a, **kw: seen.append(kw) or torch.zeros_like(a[1]))
    for overlap in (False, True):
        s = Scene()
        s.renderer(False).rasterize(CAMS, s.verts, s.faces, L, overlap=overlap)[2].sum().backward()
    assert seen == [{}, {}, {"overlap": True}, {"overlap": True}]
