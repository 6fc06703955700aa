"""What the front end (dmesh2_renderer_amd/__init__.py) hands to ``_C``, watched without a GPU.

``recording()`` replaces the ``_C.*_cuda`` entry points the front end calls with recorders that return zero tensors of the
right shapes and dtypes; ``CASES`` drive the public methods on CPU tensors (with ``verts`` on the CPU the torch projection is
taken, so nothing native loads).  Per call a recorder keeps the entry's name, its arguments bound to the entry's signature
(an explicit default equals an omitted one) and the values of the ``_C._tls`` side-channel slots at that moment;
``describe_calls`` reduces them to names, dtypes, shapes, scalars and the channels' structure -- no floating-point tensor
values -- which is what tests/golden/frontend_calls.json holds (tests/golden/make_golden.py --only-frontend-calls).
"""
import contextlib
import inspect
import itertools

import torch

import dmesh2_renderer_amd as dm
from dmesh2_renderer_amd import _C, scenes

W, H = 20, 18                       # the frame
CAMS = [1, 2]                       # two of three cameras, consecutive: the full frame's rays are views
L = 2
WINDOWS = {"full": None, "window": ([[3, 5], [7, 2]], 9, 7), "empty": ([[3, 5], [7, 2]], 0, 7)}

_CHANNELS = (_C.forward_only, _C.analytic_rays, _C.window, _C.aa_grad_to_verts, _C.tables_from_image, _C.alpha_output,
             _C.face_weights_output, _C.forward_mode)
SLOT_OFF = {c._slot: c._off for c in _CHANNELS}

RENDER_FORWARD_ARGS = [
    "background", "patch_min", "patch_width", "patch_height", "verts", "faces", "verts_color", "faces_opacity", "verts_ndc",
    "verts_image", "faces_intense", "aa_temperature", "aa_face_verts", "aa_face_edges", "aa_face_edges_iszero",
    "aa_face_edges_recip", "aa_face_edges_normal", "aa_face_edges_normal_c", "len_oarea_buffer", "image_ray_o", "image_ray_d"]
RENDER_BACKWARD_ARGS = ["num_rendered"] + RENDER_FORWARD_ARGS + [
    "dL_dout_color", "dL_dout_depth", "face_buffer", "binning_buffer", "img_buffer", "oarea", "tri_id", "tri_cnt", "doarea"]

f32, i32 = torch.float32, torch.int32


def _z(*shape, dtype=f32):
    return torch.zeros(tuple(int(s) for s in shape), dtype=dtype)


def _slot(name):
    return getattr(_C._tls, name, SLOT_OFF[name])


# -- the recorders' return values: zeros of the shapes and dtypes the entries return -------------------------------------------
def _render_forward(a):
    B, F, pw, ph = a["verts_ndc"].shape[0], a["faces"].shape[0], a["patch_width"], a["patch_height"]
    out = (0, _z(B, ph, pw, 3), _z(B, ph, pw), _z(B, ph, pw, 0), _z(B, ph, pw, 0, dtype=i32), _z(B, ph, pw, dtype=i32),
           _z(B, ph, pw, 0, 3, 2), _z(8, dtype=torch.uint8), _z(8, dtype=torch.uint8), _z(8, dtype=torch.uint8))
    if _slot("alpha_output"):
        out += (_z(B, ph, pw),)
    if _slot("face_weights_output"):
        out += (_z(B, F),)
    return out


def _render_backward(a):
    B, P, F = a["verts_ndc"].shape[0], a["verts"].shape[0], a["faces"].shape[0]
    return (_z(P, 3), _z(P, 3), _z(F), _z(B, P, 3), _z(B, F), _z(B, P, 2) if _slot("aa_to_verts") else _z(B, F, 3, 2))


def _generate(a):
    B = a["verts_ndc"].shape[0]
    return _z(B, a["height"], a["width"], a["num_layers"], dtype=i32), _z(B, a["height"], a["width"], dtype=i32)


def _rasterize(a):
    s = (a["verts_ndc"].shape[0], a["height"], a["width"], a["num_layers"])
    out = (_z(*s, dtype=i32), _z(*s[:3], dtype=i32), _z(*s, 3), _z(*s))
    return out + ((_z(*s, dtype=torch.bool),) if a["overlap"] else ())


def _shading(a):
    return tuple(_z(*a["render_layers"].shape, 3) for _ in range(2 if a["normals"] is None else 4))


def _shading_backward(a):
    return (torch.zeros_like(a["t"]) if a["need_t"] else None, torch.zeros_like(a["normals"]) if a["need_normals"] else None)


def _composite_layers(a):
    B, h, w = a["render_layers"].shape[:3]
    out = (_z(B, h, w, 3), _z(B, h, w), _z(B, h, w), _z(B, h, w, dtype=i32))
    return out + ((_z(B, a["faces"].shape[0]),) if _slot("face_weights_output") else ())


def _composite_layers_backward(a):
    B, P, F = a["verts_ndc"].shape[0], a["verts"].shape[0], a["faces"].shape[0]
    return _z(P, 3), _z(F), _z(B, P, 3), _z(B, F)


def _texture_out(a):
    uv = a["uv"] if "uv" in a else a["dirs"]
    return _z(*uv.shape[:4], a["tex"].shape[-1])


def _composite(a):
    B, h, w, _, C = a["values"].shape
    return _z(B, h, w, C), _z(B, h, w), _z(B, h, w), _z(B, h, w, dtype=i32)


FAKES = {
    "render_forward_cuda": _render_forward,
    "render_backward_cuda": _render_backward,
    "generate_render_layers_cuda": _generate,
    "rasterize_layers_cuda": _rasterize,
    "rasterize_layers_backward_cuda": lambda a: torch.zeros_like(a["verts"]),
    "coverage_cuda": lambda a: _z(*a["render_layers"].shape),
    "coverage_backward_cuda": lambda a: torch.zeros_like(a["verts_image"]),
    "bary_derivatives_cuda": lambda a: (_z(*a["render_layers"].shape, 3), _z(*a["render_layers"].shape, 3)),
    "shading_vectors_cuda": _shading,
    "shading_vectors_backward_cuda": _shading_backward,
    "composite_layers_cuda": _composite_layers,
    "composite_layers_backward_cuda": _composite_layers_backward,
    "texture_cuda": _texture_out,
    "texture_backward_cuda": lambda a: (torch.zeros_like(a["tex"]), torch.zeros_like(a["uv"])),
    "texture_cube_cuda": _texture_out,
    "texture_cube_backward_cuda": lambda a: (torch.zeros_like(a["tex"]), torch.zeros_like(a["dirs"])),
    "texture_mip_cuda": _texture_out,
    "texture_mip_backward_cuda": lambda a: (torch.zeros_like(a["tex"]), torch.zeros_like(a["mip"]), torch.zeros_like(a["uv"])),
    "composite_cuda": _composite,
    "composite_backward_cuda": lambda a: (torch.zeros_like(a["values"]), torch.zeros_like(a["alpha"])),
}
_POSITIONAL = {"render_forward_cuda": RENDER_FORWARD_ARGS, "render_backward_cuda": RENDER_BACKWARD_ARGS}


class Call:
    def __init__(self, entry, args, channels):
        self.entry, self.args, self.channels = entry, args, channels


def _recorder(name, real, calls):
    names = _POSITIONAL.get(name)
    sig = None if names else inspect.signature(real)

    def entry(*args, **kw):
        if names:                                   # (*args entries: the reference's positional lists)
            assert len(args) == len(names), (name, len(args))
            bound = dict(zip(names, args))
            if name == "render_backward_cuda":
                bound["dL_dout_alpha"] = kw.pop("dL_dout_alpha", None)
            assert not kw, kw
        else:
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            bound = dict(b.arguments)
        calls.append(Call(name, bound, {s: _slot(s) for s in SLOT_OFF}))
        return FAKES[name](bound)
    return entry


@contextlib.contextmanager
def recording():
    """``with recording() as calls:`` -- the front end's ``_C`` entries record into ``calls`` (a list of ``Call``)."""
    calls, real = [], {name: getattr(_C, name) for name in FAKES}
    for name in FAKES:
        setattr(_C, name, _recorder(name, real[name], calls))
    try:
        yield calls
    finally:
        for name in FAKES:
            setattr(_C, name, real[name])


def describe(x):
    if torch.is_tensor(x):
        return {"dtype": str(x.dtype).replace("torch.", ""), "shape": list(x.shape)}
    if isinstance(x, (tuple, list)):
        return [describe(v) for v in x]
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    raise TypeError(f"cannot describe {type(x)}")


def describe_calls(calls):
    return [{"entry": c.entry, "args": {k: describe(v) for k, v in c.args.items()},
             "channels": {k: describe(v) for k, v in c.channels.items()}} for c in calls]


# -- the scene ---------------------------------------------------------------------------------------------------------------
class Scene:
    """Five vertices, two faces, three cameras; the float inputs require grad where ``grad``."""

    def __init__(self, grad=True):
        cams = [scenes.camera(W, H, shift) for shift in ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1), (-0.25, 0.15, 0.0))]
        self.mv, self.proj = torch.stack([c[0] for c in cams]), torch.stack([c[1] for c in cams])
        leaf = lambda rows: torch.tensor(rows, dtype=f32).requires_grad_(grad)
        self.verts = leaf([[-0.8, -0.6, 0.1], [0.7, -0.5, -0.2], [0.1, 0.8, 0.0], [0.9, 0.6, 0.3], [-0.4, 0.5, -0.3]])
        self.faces = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=i32)
        self.verts_color = leaf([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9], [0.2, 0.4, 0.6], [0.9, 0.5, 0.1]])
        self.faces_opacity = leaf([0.6, 0.8])
        self.faces_intense = leaf([[1.0, 0.9], [0.8, 0.7]])          # (B,F) of the selected views
        self.background = torch.tensor([0.1, 0.2, 0.3], dtype=f32)
        self.faces_existence = torch.tensor([1, 1], dtype=i32)
        self.tets = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=i32)
        self.face_tets = torch.tensor([[0, -1], [1, -1]], dtype=i32)
        self.tet_faces = torch.tensor([[0, -1, -1, -1], [1, -1, -1, -1]], dtype=i32)

    def renderer(self, analytic, layered=False, **kw):
        cls = dm.LayeredRenderer if layered else dm.Renderer
        return cls(self.mv, self.proj, W, H, "cpu", analytic_rays=analytic, **kw)


def window_args(win, sized=True):
    """The keyword arguments of a window: ``patch_min`` (with the sizes where the method takes them)."""
    if WINDOWS[win] is None:
        return {}
    pm, pw, ph = WINDOWS[win]
    kw = {"patch_min": torch.tensor(pm, dtype=i32)}
    if sized:
        kw.update(patch_width=pw, patch_height=ph)
    return kw


def window_size(win):
    return (W, H) if WINDOWS[win] is None else WINDOWS[win][1:]


def layers_of(win, cams=CAMS):
    pw, ph = window_size(win)
    return torch.zeros((len(cams), ph, pw, L), dtype=i32)


def _backwards(losses, leaves):
    """One backward per loss (a list of output tensors, summed), in order, on the same forward."""
    for outs in losses:
        outs = [o for o in outs if o.requires_grad]
        if outs:
            torch.autograd.grad(sum(o.sum() for o in outs), leaves, retain_graph=True, allow_unused=True)


# -- the cases: name -> thunk driving one public method, forward and backwards -----------------------------------------------
def _forward_case(analytic, win, alpha, weights, **renderer_kw):
    def run():
        s = Scene()
        r = s.renderer(analytic, **renderer_kw)
        pm, pw, ph = ([[0, 0], [0, 0]], W, H) if WINDOWS[win] is None else WINDOWS[win]
        out = r(CAMS, torch.tensor(pm, dtype=i32), pw, ph, s.verts, s.faces, s.verts_color, s.faces_opacity, s.faces_intense,
                s.background, aa_temperature=0.5, return_alpha=alpha, return_face_weights=weights)
        leaves = [s.verts, s.verts_color, s.faces_opacity, s.faces_intense]
        # all outputs; the colour alone; under alpha: alpha alone (colour and depth gradients arrive unmaterialised)
        _backwards([out[:3 if alpha else 2], out[:1]] + ([out[2:3]] if alpha else []), leaves)
    return run


def _rasterize_case(analytic, win, overlap, existence=False, cams=CAMS):
    def run():
        s = Scene()
        out = s.renderer(analytic).rasterize(cams, s.verts, s.faces, L, faces_existence=s.faces_existence if existence else None,
                                             overlap=overlap, **window_args(win))
        _backwards([out[2:4], out[3:4]], [s.verts])
    return run


def _coverage_case(analytic, win, inside=False):
    def run():
        s = Scene()
        rl = layers_of(win)
        cov = s.renderer(analytic).coverage(CAMS, rl, s.verts, s.faces, temperature=0.5, inside=torch.ones_like(rl) if inside else None,
                                            **window_args(win, sized=False))
        _backwards([[cov]], [s.verts])
    return run


def _bary_case(analytic, win):
    def run():
        s = Scene()
        s.renderer(analytic).bary_derivatives(CAMS, layers_of(win), s.verts, s.faces, **window_args(win, sized=False))
    return run


def _shading_case(analytic, win, normals):
    def run():
        s = Scene()
        rl = layers_of(win)
        t = torch.ones(tuple(rl.shape), dtype=f32, requires_grad=True)
        n = torch.ones(tuple(rl.shape) + (3,), dtype=f32, requires_grad=True) if normals else None
        out = s.renderer(analytic).shading_vectors(CAMS, rl, t, n, **window_args(win, sized=False))
        _backwards([out, out[:1]] + ([out[3:]] if normals else []), [t] + ([n] if normals else []))
    return run


def _generate_case(analytic, win):
    def run():
        s = Scene(grad=False)
        s.renderer(analytic, layered=True).generate(CAMS, s.verts, s.faces, s.tets, s.face_tets, s.tet_faces, s.faces_existence, L,
                                                    **window_args(win))
    return run


def _render_case(analytic, win, alpha, weights):
    def run():
        s = Scene()
        out = s.renderer(analytic, layered=True).render(CAMS, layers_of(win), s.verts, s.faces, s.verts_color, s.faces_opacity,
                                                        s.faces_intense, s.background, return_alpha=alpha,
                                                        return_face_weights=weights, **window_args(win, sized=False))
        _backwards([out[:3 if alpha else 2], out[:1]] + ([out[2:3]] if alpha else []),
                   [s.verts, s.verts_color, s.faces_opacity, s.faces_intense])
    return run


def _texture_case(kind, layers):
    """The ops whose Functions save a tensor that may be None: texture (plain, cube, mip) and composite."""
    def run():
        r = Scene().renderer(False)
        rl = layers_of("window") if layers else None
        shape = tuple(layers_of("window").shape)
        leaf = lambda *s: torch.ones(s, dtype=f32, requires_grad=True)
        if kind == "composite":
            values, alpha = leaf(*shape, 3), leaf(*shape)
            out = r.composite(values, alpha, rl, torch.ones(3) if layers else None)
            _backwards([out, out[1:]], [values, alpha])
            return
        tex = leaf(6, 4, 4, 3) if kind == "cube" else leaf(4, 4, 3)
        uv = leaf(*shape, 3 if kind == "cube" else 2)
        if kind == "mip":
            out = r.texture(uv, tex, rl, filter_mode="linear-mipmap-linear", uv_da=torch.ones(shape + (4,)), mip=leaf(5, 3))
        else:
            out = r.texture(uv, tex, rl, boundary_mode="cube" if kind == "cube" else "wrap")
        _backwards([[out]], [uv, tex])
    return run


def _cases():
    c = {}
    both, wins = (False, True), tuple(WINDOWS)
    for ana, win, (alpha, weights) in itertools.product(both, wins, itertools.product(both, both)):      # (empty: forward has no early-out)
        c[f"forward-{win}-ana{int(ana)}-alpha{int(alpha)}-weights{int(weights)}"] = _forward_case(ana, win, alpha, weights)
    # the three prep routes of forward, as far as they run on CPU tensors: each takes the torch projection
    c["forward-full-unfused"] = _forward_case(False, "full", False, False, fused_prep=False)
    c["forward-full-materialised-tables"] = _forward_case(False, "full", False, False, fused_prep=True, tables_from_image=False)
    c["forward-full-tables-from-image"] = _forward_case(False, "full", False, False, fused_prep=True, tables_from_image=True)
    for ana, win in itertools.product(both, wins):
        k = f"{win}-ana{int(ana)}"
        for overlap in both:
            c[f"rasterize-overlap{int(overlap)}-{k}"] = _rasterize_case(ana, win, overlap)
        c[f"coverage-{k}"] = _coverage_case(ana, win)
        c[f"bary_derivatives-{k}"] = _bary_case(ana, win)
        for normals in both:
            c[f"shading_vectors-normals{int(normals)}-{k}"] = _shading_case(ana, win, normals)
        c[f"generate-{k}"] = _generate_case(ana, win)
        for alpha, weights in itertools.product(both, both):
            c[f"render-{k}-alpha{int(alpha)}-weights{int(weights)}"] = _render_case(ana, win, alpha, weights)
    c["rasterize-existence-full"] = _rasterize_case(False, "full", False, existence=True)
    c["rasterize-scattered-cameras-full"] = _rasterize_case(False, "full", False, cams=[2, 0])
    c["rasterize-scattered-cameras-window-ana1"] = _rasterize_case(True, "window", True, cams=[2, 0])
    c["coverage-inside-window"] = _coverage_case(False, "window", inside=True)
    for kind, layers in itertools.product(("plain", "cube", "mip", "composite"), both):
        c[f"texture-{kind}-layers{int(layers)}" if kind != "composite" else f"composite-layers{int(layers)}"] = _texture_case(kind, layers)
    return c


CASES = _cases()


def run_case(name):
    with recording() as calls:
        CASES[name]()
    return calls


def trace():
    """name -> the described calls of every case: the content of tests/golden/frontend_calls.json."""
    return {name: describe_calls(run_case(name)) for name in CASES}
