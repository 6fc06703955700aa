"""What the shim (dmesh2_renderer_amd/_C.py) hands to the native library for the per-slot lookup ops, watched without a GPU.

Two records, both plain data (tests/golden/make_golden.py --only-shim-errors / --only-shim-calls):

``errors()``   malformed arguments -> the exception's type and whole message, twice per case: ``raw`` on plain CPU tensors
               (where the "no CPU path" error comes once every shape and mode check has passed) and ``traced`` inside
               ``recording()`` (where ``_require_gpu`` passes, so the dtype checks and whatever sits behind them are reached;
               None where the call goes through).
``calls()``    inside ``recording()`` the library is a recorder: per export called, its name, every integer argument and per
               pointer argument null or the role, dtype and shape of the tensor it points to (matched by ``data_ptr()``
               against the call's inputs and what it returned); plus dtype and shape of what the entry returned.

The recorder cannot tell ``torch.zeros`` from ``torch.empty``; the GPU suites' "every element written" and accumulation tests
hold those.
"""
import contextlib
import ctypes
import inspect
import itertools

import torch

from dmesh2_renderer_amd import _C

f32, f64, f16, i32, i64 = torch.float32, torch.float64, torch.float16, torch.int32, torch.int64
B, H, W, L = 2, 4, 5, 3
STREAM = 0x57                     # what the patched ``_C._stream`` hands out


def _z(*shape, dtype=f32):
    return torch.zeros(tuple(shape), dtype=dtype)


def _huge(*shape):
    """A tensor of that shape without memory (the meta device): the 2^31 bounds are shape checks, nothing is read."""
    return torch.zeros(tuple(shape), device="meta")


# -- the recorder ---------------------------------------------------------------------------------------------------------------
class _Library:
    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        if name not in _C.EXPORTS:
            raise AttributeError(name)

        def export(*args):
            self._calls.append((name, [a.value if isinstance(a, ctypes.c_void_p) else a for a in args],
                                [isinstance(a, ctypes.c_void_p) for a in args]))
            return 0
        return export


@contextlib.contextmanager
def recording():
    """``with recording() as calls:`` -- the shim runs on CPU tensors and the library's exports record into ``calls``."""
    calls = []
    lib = _Library(calls)
    real = (_C.load_library, _C._require_gpu, _C._stream, torch.cuda.device)
    _C.load_library = lambda path=None: lib
    _C._require_gpu = lambda *tensors: tensors[0].device
    _C._stream = lambda dev: ctypes.c_void_p(STREAM)
    torch.cuda.device = lambda dev: contextlib.nullcontext()
    try:
        yield calls
    finally:
        _C.load_library, _C._require_gpu, _C._stream, torch.cuda.device = real


def _tensor(t):
    return None if t is None else f"{str(t.dtype).replace('torch.', '')}{list(t.shape)}"


def _describe(calls, roles):
    """roles: name -> tensor.  A pointer is null, the stream, ``role:dtype[shape]`` or ``?`` (a buffer of the shim's own)."""
    by_ptr = {t.data_ptr(): f"{name}:{_tensor(t)}" for name, t in roles.items() if t is not None and t.numel() > 0}
    out = []
    for name, args, is_ptr in calls:
        words = []
        for a, p in zip(args, is_ptr):
            if not p:
                assert isinstance(a, int), (name, a)
                words.append(a)
            else:
                words.append(None if not a else "stream" if a == STREAM else by_ptr.get(a, "?"))
        out.append({"export": name, "args": words})
    return out


# -- the ops --------------------------------------------------------------------------------------------------------------------
class Op:
    """fwd / bwd: the ``_C`` entries; inputs(per_view, h): name -> tensor, in the entries' order, up to render_layers;
    modes: name -> values to sweep (the first is the default); grads: the names of what the backward returns; C: channels."""

    def __init__(self, fwd, bwd, inputs, modes, grads, C=3, per_view=(False, True)):
        self.fwd, self.bwd, self.inputs, self.modes, self.grads, self.C, self.per_view = fwd, bwd, inputs, modes, grads, C, per_view
        self.names = list(inspect.signature(getattr(_C, bwd)).parameters)
        self.needs = [n for n in self.names if n.startswith("need_")]
        assert list(inspect.signature(getattr(_C, fwd)).parameters) == self.names[:self.names.index("grad_out")]

    def args(self, per_view=False, layers=True, h=H, **over):
        a = dict(self.inputs(per_view, h))
        a["render_layers"] = _z(B, h, W, L, dtype=i32) if layers else None
        a.update({k: v[0] for k, v in self.modes.items()})
        a["grad_out"] = _z(B, h, W, L, self.C)
        a.update({n: True for n in self.needs})
        assert set(over) <= set(a), over
        a.update(over)
        return a

    def call(self, backward, a):
        """-> (the entry's return as a tuple, name -> tensor of everything that went in or came out)."""
        names = self.names if backward else self.names[:self.names.index("grad_out")]
        ret = getattr(_C, self.bwd if backward else self.fwd)(*[a[n] for n in names])
        ret = ret if backward else (ret,)
        roles = {n: a[n] for n in names if torch.is_tensor(a[n])}
        roles.update(zip(self.grads if backward else ("out",), ret))
        return ret, roles


def _pv(per_view, *shape):
    return _z(*((B,) if per_view else ()), *shape)


OPS = {
    "texture": Op("texture_cuda", "texture_backward_cuda",
                  lambda pv, h: {"uv": _z(B, h, W, L, 2), "tex": _pv(pv, 4, 4, 3)},
                  {"filter_mode": ["linear", "nearest"], "boundary_mode": ["wrap", "clamp"]}, ("dL_dtex", "dL_duv")),
    "texture_cube": Op("texture_cube_cuda", "texture_cube_backward_cuda",
                       lambda pv, h: {"dirs": _z(B, h, W, L, 3), "tex": _pv(pv, 6, 4, 4, 3)},
                       {"filter_mode": ["linear", "nearest"]}, ("dL_dtex", "dL_ddirs")),
    "texture_volume": Op("texture_volume_cuda", "texture_volume_backward_cuda",
                         lambda pv, h: {"xyz": _z(B, h, W, L, 3), "grid": _pv(pv, 4, 4, 4, 3)},
                         {"filter_mode": ["linear", "nearest"], "boundary_mode": ["clamp", "wrap"]}, ("dL_dgrid", "dL_dxyz")),
    "hash_grid": Op("hash_grid_cuda", "hash_grid_backward_cuda",
                    lambda pv, h: {"xyz": _z(B, h, W, L, 3), "table": _z(4, 64, 2)},
                    {"base_resolution": [16, 5], "growth": [1.5, 2.0], "filter_mode": ["linear", "nearest"],
                     "boundary_mode": ["clamp", "wrap"]}, ("dL_dtable", "dL_dxyz"), C=8, per_view=(False,)),
    "texture_mip": Op("texture_mip_cuda", "texture_mip_backward_cuda",
                      lambda pv, h: {"uv": _z(B, h, W, L, 2), "uv_da": _z(B, h, W, L, 4), "tex": _pv(pv, 4, 4, 3), "mip": _pv(pv, 5, 3)},
                      {"boundary_mode": ["wrap", "clamp"], "max_mip_level": [None]}, ("dL_dtex", "dL_dmip", "dL_duv")),
    "texture_cube_mip": Op("texture_cube_mip_cuda", "texture_cube_mip_backward_cuda",
                           lambda pv, h: {"dirs": _z(B, h, W, L, 3), "level": _z(B, h, W, L), "tex": _pv(pv, 6, 4, 4, 3),
                                          "mip": _pv(pv, 6, 5, 3)},
                           {"max_mip_level": [None]}, ("dL_dtex", "dL_dmip", "dL_ddirs", "dL_dlevel")),
}
# a chain cut short: the level limit reaches the library as a word of its own
MIP_LIMITED = {"texture_mip": {"max_mip_level": 1, "mip": _z(4, 3)}, "texture_cube_mip": {"max_mip_level": 1, "mip": _z(6, 4, 3)}}


def _flag_sets(op):
    """Each single need_* flag, all of them, none of them."""
    n = len(op.needs)
    sets = [tuple(i == j for i in range(n)) for j in range(n)] + [(True,) * n, (False,) * n]
    return [dict(zip(op.needs, s)) for s in sets]


def _label(d):
    """need_tex=True -> "+tex" (False: left out), filter_mode="linear" -> "filter_mode=linear"."""
    return ",".join(k.replace("need_", "+") if v is True else f"{k}={v}" for k, v in d.items() if v is not False) or "nothing"


def _trace_one(op, backward, a):
    with recording() as calls:
        ret, roles = op.call(backward, a)
    return {"calls": _describe(calls, roles), "returns": [_tensor(t) for t in ret]}


def calls():
    """case name -> {"calls": the described library calls, "returns": dtype and shape of what the entry returned}."""
    out = {}
    for name, op in OPS.items():
        sweeps = [dict(zip(op.modes, vs)) for vs in itertools.product(*op.modes.values())]
        for modes, pv, layers in itertools.product(sweeps, op.per_view, (True, False)):
            tag = f"{_label(modes)}-per_view{int(pv)}-layers{int(layers)}"
            out[f"{name}-forward-{tag}"] = _trace_one(op, False, op.args(pv, layers, **modes))
            out[f"{name}-backward-{tag}"] = _trace_one(op, True, op.args(pv, layers, **modes))
        for flags, pv, layers in itertools.product(_flag_sets(op)[:-2] + _flag_sets(op)[-1:], op.per_view, (True, False)):
            out[f"{name}-backward-{_label(flags)}-per_view{int(pv)}-layers{int(layers)}"] = _trace_one(op, True, op.args(pv, layers, **flags))
        for flags in _flag_sets(op)[:-2]:                      # a nearest filter's coordinate gradient is the library's to zero
            if "filter_mode" in op.modes:
                out[f"{name}-backward-nearest-{_label(flags)}"] = _trace_one(op, True, op.args(filter_mode="nearest", **flags))
        for pv in op.per_view:                                 # the empty grid: no call, what comes back instead
            out[f"{name}-forward-empty-per_view{int(pv)}"] = _trace_one(op, False, op.args(pv, True, h=0))
            for flags in _flag_sets(op):
                out[f"{name}-backward-empty-{_label(flags)}-per_view{int(pv)}"] = _trace_one(op, True, op.args(pv, True, h=0, **flags))
        if name in MIP_LIMITED:
            out[f"{name}-forward-limited"] = _trace_one(op, False, op.args(**MIP_LIMITED[name]))
            out[f"{name}-backward-limited"] = _trace_one(op, True, op.args(**MIP_LIMITED[name]))
    for label, fn, args, roles in _chain_calls():
        with recording() as rec:
            ret = fn(*args)
        out[label] = {"calls": _describe(rec, dict(roles, out=ret)), "returns": [_tensor(ret)]}
    return out


def _chain_calls():
    for pv, level in itertools.product((False, True), (None, 1, 0)):
        tex, T = _pv(pv, 4, 4, 3), {None: 5, 1: 4, 0: 0}[level]
        tag = f"max_mip_level={level}-per_view{int(pv)}"
        yield f"texture_mipmaps-forward-{tag}", _C.texture_mipmaps_cuda, (tex, level), {"tex": tex}
        g = _pv(pv, T, 3)
        yield f"texture_mipmaps-backward-{tag}", _C.texture_mipmaps_backward_cuda, (tex, level, g), {"tex": tex, "grad_mip": g}
        chain = _pv(pv, 6, T, 3)
        yield f"cube_prefilter-forward-{tag}", _C.cube_prefilter_cuda, (chain, 4, level), {"chain": chain}
        yield f"cube_prefilter-transpose-{tag}", _C.cube_prefilter_transpose_cuda, (chain, 4, level), {"grad": chain}


# -- the error table --------------------------------------------------------------------------------------------------------------
def _slots(*tail, dtype=f32):
    return _z(B, H, W, L, *tail, dtype=dtype)


_COMMON = {                       # (the coordinate's name and the table's are filled in per op)
    "valid": {},
    "filter": {"filter_mode": "cubic"},
    "coord-rank": {"{x}": _z(B, H, W, L)},
    "coord-width": {"{x}": _slots(5)},
    "layers-shape": {"render_layers": _z(B, H, W, 2, dtype=i32)},
    "grad_out-shape": {"grad_out": _slots(11)},
    "coord-dtype": {"{x}": "f64"},
    "table-dtype": {"{t}": "f16"},
    "layers-dtype": {"render_layers": "i64"},
    "grad_out-dtype": {"grad_out": "f64"},
    "filter+coord-rank": {"filter_mode": None, "{x}": _z(B, H, W, L)},
    "coord-width+layers-shape": {"{x}": _slots(5), "render_layers": _z(B, H, W, dtype=i32)},
    "layers-shape+grad_out-shape": {"render_layers": _z(1, H, W, L, dtype=i32), "grad_out": _slots()},
    "grad_out-shape+coord-dtype": {"grad_out": _slots(11), "{x}": "f64"},
    "coord-dtype+table-dtype": {"{x}": "i32", "{t}": "f64"},
    "layers-dtype+grad_out-dtype": {"render_layers": "f32", "grad_out": "f16"},
}
_BOUNDARY = {
    "boundary": {"boundary_mode": "mirror"},
    "filter+boundary": {"filter_mode": "cubic", "boundary_mode": "cube"},
    "boundary+coord-rank": {"boundary_mode": None, "{x}": _z(B, H, W)},
}
_ERRORS = {
    "texture": ("uv", "tex", dict(_COMMON, **_BOUNDARY, **{
        "table-rank": {"tex": _z(4, 3)}, "table-views": {"tex": _z(3, 4, 4, 3)}, "table-rows": {"tex": _z(0, 4, 3)},
        "table-columns": {"tex": _z(4, 0, 3)}, "table-channels": {"tex": _z(4, 4, 0)}, "table-2^31": {"tex": _huge(2 ** 16, 2 ** 15, 3)},
        "coord-width+table-rank": {"uv": _slots(3), "tex": _z(4)}, "table-views+table-channels": {"tex": _z(3, 4, 4, 0)},
        "table-rows+table-channels": {"tex": _z(0, 4, 0)}, "table-channels+layers-shape": {"tex": _z(4, 4, 0), "render_layers": _z(B, dtype=i32)},
        "table-2^31+grad_out-shape": {"tex": _huge(2 ** 16, 2 ** 15, 3), "grad_out": _slots(3)}})),
    "texture_cube": ("dirs", "tex", dict(_COMMON, **{
        "table-rank": {"tex": _z(6, 4, 3)}, "table-views": {"tex": _z(3, 6, 4, 4, 3)}, "table-faces": {"tex": _z(5, 4, 4, 3)},
        "table-square": {"tex": _z(6, 4, 5, 3)}, "table-rows": {"tex": _z(6, 0, 0, 3)}, "table-channels": {"tex": _z(6, 4, 4, 0)},
        "table-2^31": {"tex": _huge(6, 18919, 18919, 3)},
        "coord-width+table-rank": {"dirs": _slots(2), "tex": _z(4)}, "table-views+table-faces": {"tex": _z(3, 5, 4, 4, 3)},
        "table-faces+table-square": {"tex": _z(5, 4, 5, 3)}, "table-square+table-channels": {"tex": _z(6, 5, 4, 0)},
        "table-rows+table-channels": {"tex": _z(6, 0, 0, 0)}, "table-2^31+layers-shape": {"tex": _huge(6, 18919, 18919, 3), "render_layers": _z(B, dtype=i32)}})),
    "texture_volume": ("xyz", "grid", dict(_COMMON, **_BOUNDARY, **{
        "table-rank": {"grid": _z(4, 4, 3)}, "table-views": {"grid": _z(3, 4, 4, 4, 3)}, "table-cube": {"grid": _z(4, 5, 4, 3)},
        "table-cube-k": {"grid": _z(5, 4, 4, 3)}, "table-voxels": {"grid": _z(0, 0, 0, 3)}, "table-channels": {"grid": _z(4, 4, 4, 0)},
        "table-2^31": {"grid": _huge(1291, 1291, 1291, 3)},
        "coord-width+table-rank": {"xyz": _slots(2), "grid": _z(4)}, "table-views+table-cube": {"grid": _z(3, 4, 5, 4, 3)},
        "table-cube+table-channels": {"grid": _z(4, 4, 5, 0)}, "table-voxels+table-channels": {"grid": _z(0, 0, 0, 0)},
        "table-2^31+layers-shape": {"grid": _huge(1291, 1291, 1291, 3), "render_layers": _z(B, dtype=i32)}})),
    "hash_grid": ("xyz", "table", dict(_COMMON, **_BOUNDARY, **{
        "table-rank": {"table": _z(64, 2)}, "table-no-levels": {"table": _z(0, 64, 2)}, "table-levels": {"table": _z(33, 64, 2)},
        "table-rows-power": {"table": _z(4, 48, 2)}, "table-rows-few": {"table": _z(4, 8, 2)}, "table-rows-none": {"table": _z(4, 0, 2)},
        "table-features": {"table": _z(4, 64, 3)}, "table-2^31": {"table": _huge(32, 2 ** 24, 8)},
        "growth": {"growth": 1.51}, "growth-nan": {"growth": float("nan")}, "growth-small": {"growth": 1.0},
        "base_resolution": {"base_resolution": 0}, "finest": {"base_resolution": 2 ** 20}, "grad_out-channels": {"grad_out": _slots(4)},
        "coord-width+table-rank": {"xyz": _slots(2), "table": _z(4)}, "table-levels+table-rows": {"table": _z(33, 48, 2)},
        "table-rows+table-features": {"table": _z(4, 48, 3)}, "table-features+growth": {"table": _z(4, 64, 3), "growth": 3.0},
        "growth+base_resolution": {"growth": 1.51, "base_resolution": 0}, "base_resolution+layers-shape":
        {"base_resolution": -1, "render_layers": _z(B, dtype=i32)}, "finest+grad_out-shape": {"base_resolution": 2 ** 20, "grad_out": _slots(3)}})),
    "texture_mip": ("uv", "tex", dict({k: v for k, v in _COMMON.items() if "filter" not in k}, **{
        "boundary": {"boundary_mode": "mirror"}, "boundary+coord-rank": {"boundary_mode": "cube", "uv": _z(B, H, W)},
        "table-rank": {"tex": _z(4, 3)}, "table-views": {"tex": _z(3, 4, 4, 3)}, "table-channels": {"tex": _z(4, 4, 0)},
        "uv_da-shape": {"uv_da": _slots(2)}, "chain-2^31": {"tex": _huge(2 ** 16, 28672, 3)}, "mip-shape": {"mip": _z(4, 3)},
        "mip-views": {"mip": _z(B, 5, 3)}, "max_mip_level": {"max_mip_level": -1}, "uv_da-dtype": {"uv_da": "f64"}, "mip-dtype": {"mip": "f16"},
        "grad_out-shape+uv_da-shape": {"grad_out": _slots(11), "uv_da": _slots(2)}, "coord-dtype+uv_da-shape": {"uv": "f64", "uv_da": _slots(2)},
        "uv_da-shape+chain-2^31": {"uv_da": _slots(2), "tex": _huge(2 ** 16, 28672, 3)}, "uv_da-shape+max_mip_level": {"uv_da": _slots(), "max_mip_level": -1},
        "chain-2^31+mip-shape": {"tex": _huge(2 ** 16, 28672, 3), "mip": _z(3)}, "mip-shape+uv_da-dtype": {"mip": _z(4, 3), "uv_da": "f64"},
        "uv_da-dtype+mip-dtype": {"uv_da": "f16", "mip": "f64"}})),
    "texture_cube_mip": ("dirs", "tex", dict({k: v for k, v in _COMMON.items() if "filter" not in k}, **{
        "table-rank": {"tex": _z(6, 4, 3)}, "table-faces": {"tex": _z(5, 4, 4, 3)}, "table-square": {"tex": _z(6, 4, 5, 3)},
        "table-channels": {"tex": _z(6, 4, 4, 0)}, "level-shape": {"level": _slots(1)}, "chain-2^31": {"tex": _huge(6, 18000, 18000, 3)},
        "mip-shape": {"mip": _z(5, 3)}, "mip-views": {"mip": _z(B, 6, 5, 3)}, "max_mip_level": {"max_mip_level": -1},
        "level-dtype": {"level": "f64"}, "mip-dtype": {"mip": "f16"},
        "grad_out-shape+level-shape": {"grad_out": _slots(11), "level": _slots(1)}, "coord-dtype+level-shape": {"dirs": "f64", "level": _slots(1)},
        "level-shape+chain-2^31": {"level": _z(B), "tex": _huge(6, 18000, 18000, 3)}, "level-shape+max_mip_level": {"level": _z(B), "max_mip_level": -1},
        "chain-2^31+mip-shape": {"tex": _huge(6, 18000, 18000, 3), "mip": _z(3)}, "mip-shape+level-dtype": {"mip": _z(6, 4, 3), "level": "f64"},
        "level-dtype+mip-dtype": {"level": "f16", "mip": "f64"}})),
}
_DTYPES = {"f64": f64, "f16": f16, "f32": f32, "i32": i32, "i64": i64}


def _raised(thunk):
    try:
        thunk()
    except Exception as e:              # noqa: BLE001 -- the type is what is recorded
        return [type(e).__name__, str(e)]
    return None


def _both(thunk):
    raw = _raised(thunk)
    with recording():
        traced = _raised(thunk)
    return {"raw": raw, "traced": traced}


def _chain_errors():
    tex, chain = _z(4, 4, 3), _z(6, 5, 3)
    mm = {
        "valid": (tex, None, _z(5, 3)), "table-rank": (_z(4, 3), None, _z(5, 3)), "table-rows": (_z(0, 4, 3), None, _z(0, 3)),
        "table-channels": (_z(4, 4, 0), None, _z(5, 0)), "max_mip_level": (tex, -1, _z(5, 3)), "chain-2^31": (_huge(2 ** 16, 28672, 3), None, _z(5, 1)),
        "grad_mip-shape": (tex, None, _z(4, 3)), "grad_mip-views": (_z(B, 4, 4, 3), None, _z(5, 3)), "table-dtype": (tex.to(f64), None, _z(5, 3)),
        "grad_mip-dtype": (tex, None, _z(5, 3, dtype=f16)), "table-rank+max_mip_level": (_z(4), -1, _z(5, 3)),
        "table-rows+table-channels": (_z(4, 0, 0), None, _z(5, 3)), "table-channels+max_mip_level": (_z(4, 4, 0), -1, _z(5, 3)),
        "max_mip_level+grad_mip-shape": (tex, -1, _z(4, 3)), "chain-2^31+grad_mip-shape": (_huge(2 ** 16, 28672, 3), None, _z(5, 3)),
        "grad_mip-shape+table-dtype": (tex.to(f64), None, _z(4, 3)), "table-dtype+grad_mip-dtype": (tex.to(f16), None, _z(5, 3, dtype=f64)),
    }
    for label, (t, level, g) in mm.items():
        if "grad_mip" not in label:
            yield f"texture_mipmaps-forward-{label}", lambda t=t, level=level: _C.texture_mipmaps_cuda(t, level)
        yield f"texture_mipmaps-backward-{label}", lambda t=t, level=level, g=g: _C.texture_mipmaps_backward_cuda(t, level, g)
    cp = {
        "valid": (chain, 4, None), "N": (chain, 0, None), "chain-rank": (_z(5, 3), 4, None), "chain-faces": (_z(5, 5, 3), 4, None),
        "chain-2^31": (_z(6, 1, 1), 18000, None), "chain-texels": (_z(6, 4, 3), 4, None), "chain-limited": (chain, 4, 1),
        "chain-channels": (_z(6, 5, 0), 4, None), "max_mip_level": (chain, 4, -1), "chain-dtype": (chain.to(f64), 4, None),
        "chain-cubes": (_z(10923, 6, 5, 3), 4, None), "N+chain-rank": (_z(5, 3), -2, None),
        "chain-rank+chain-faces": (_z(5), 4, None), "chain-faces+max_mip_level": (_z(5, 5, 3), 4, -1), "max_mip_level+chain-texels": (_z(6, 4, 3), 4, -1),
        "chain-2^31+chain-texels": (_z(6, 1, 0), 18000, None), "chain-texels+chain-channels": (_z(6, 4, 0), 4, None),
        "chain-channels+chain-dtype": (_z(6, 5, 0, dtype=f64), 4, None), "chain-dtype+chain-cubes": (_z(10923, 6, 5, 3, dtype=f64), 4, None),
    }
    for label, a in cp.items():
        yield f"cube_prefilter-forward-{label}", lambda a=a: _C.cube_prefilter_cuda(*a)
        yield f"cube_prefilter-transpose-{label}", lambda a=a: _C.cube_prefilter_transpose_cuda(*a)


def errors():
    """case name -> {"raw": [type, message] on CPU tensors, "traced": [type, message] or None inside ``recording()``}."""
    out = {}
    for name, (x, t, table) in _ERRORS.items():
        op = OPS[name]
        for label, over in table.items():
            over = {k.format(x=x, t=t): v for k, v in over.items()}
            good = op.args()
            a = dict(good, **{k: good[k].to(_DTYPES[v]) if isinstance(v, str) and v in _DTYPES else v for k, v in over.items()})
            if not any(k.startswith("grad_out") for k in over):
                out[f"{name}-forward-{label}"] = _both(lambda: op.call(False, a))
            out[f"{name}-backward-{label}"] = _both(lambda: op.call(True, a))
    for label, thunk in _chain_errors():
        out[label] = _both(thunk)
    return out
