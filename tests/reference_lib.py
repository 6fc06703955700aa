"""The reference project's own kernels, built for gfx950 by oracle/build_ref.py into oracle/_ref/ (two Python modules):
loading them, calling them, and reading the byte buffers their forward returns.

``load(variant)`` -> the module (``render_forward_cuda``, ``render_backward_cuda``, ``generate_render_layers_cuda`` with the
reference's own 21 / 31 / 13 positional arguments), or None when oracle/_ref/MANIFEST.json is absent.  Importing needs no GPU;
calling does.  torch is imported first (the modules link against its libraries and carry no rpath), then the module is loaded
by path.
"""
import importlib.machinery
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
MANIFEST = os.path.join(REF_DIR, "MANIFEST.json")
VARIANTS = ("strict", "shipped")
ENTRY_POINTS = ("render_forward_cuda", "render_backward_cuda", "generate_render_layers_cuda")
ALIGN = 128                                   # every array of a state is carved at this alignment

_loaded = {}


def manifest():
    if not os.path.isfile(MANIFEST):
        return None
    with open(MANIFEST) as f:
        return json.load(f)


def load(variant="strict"):
    if variant in _loaded:
        return _loaded[variant]
    m = manifest()
    if m is None:
        return None
    import torch  # noqa: F401  (its shared libraries must be in the process before the module's)
    path = os.path.join(REF_DIR, m["modules"][variant])
    name = "dm2_ref_" + variant
    spec = importlib.util.spec_from_file_location(name, path, loader=importlib.machinery.ExtensionFileLoader(name, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules[name] = mod
    _loaded[variant] = mod
    return mod


# ---- the forward's byte buffers ------------------------------------------------------------------------------------------
def _carve(buf, sizes):
    """Offsets (bytes from the buffer's start) of consecutive arrays of ``sizes`` bytes, each begun at the next address that is
    a multiple of ALIGN."""
    base = buf.data_ptr()
    p, out = base, []
    for s in sizes:
        p = (p + ALIGN - 1) // ALIGN * ALIGN
        out.append(p - base)
        p += s
    return out


def _view(buf, off, count, dtype):
    return buf[off:off + count * np.dtype(dtype).itemsize].cpu().numpy().view(dtype)


def image_state(image_buffer, B, H, W):
    """-> dict(final_T (N) f32, final_prev_T (N) f32, n_contrib (N) u32, ranges (tiles, 2) u32) of a forward's image buffer:
    four arrays of N = B*H*W entries in that order (ranges has 8-byte entries, of which the first B * tiles are used)."""
    N = B * H * W
    Tn = B * ((W + 15) // 16) * ((H + 15) // 16)
    if image_buffer.numel() == 0:
        return None
    o = _carve(image_buffer, [4 * N, 4 * N, 4 * N, 8 * N])
    return dict(final_T=_view(image_buffer, o[0], N, np.float32), final_prev_T=_view(image_buffer, o[1], N, np.float32),
                n_contrib=_view(image_buffer, o[2], N, np.uint32),
                ranges=_view(image_buffer, o[3], 2 * Tn, np.uint32).reshape(Tn, 2))


def face_list(binning_buffer, num_rendered):
    """The sorted face list: the first ``num_rendered`` uint32 of a forward's binning buffer."""
    if num_rendered == 0 or binning_buffer.numel() == 0:
        return np.zeros(0, np.uint32)
    o = _carve(binning_buffer, [4 * num_rendered])
    return _view(binning_buffer, o[0], num_rendered, np.uint32)


# ---- calls -----------------------------------------------------------------------------------------------------------------
def to_device(args, dev="cuda:0"):
    import torch
    return [a.to(dev) if torch.is_tensor(a) else a for a in args]


class Forward:
    """A reference forward's outputs as numpy arrays (and the device tuple ``out`` its backward wants)."""

    def __init__(self, mod, dargs):
        import torch
        self.dargs = dargs
        _defined(dargs[5], dargs[8], dargs[9], dargs[1], int(dargs[2]), int(dargs[3]))
        out = self.out = mod.render_forward_cuda(*dargs)
        torch.cuda.synchronize()
        self.num_rendered = int(out[0])
        self.color, self.depth = out[1].cpu().numpy(), out[2].cpu().numpy()
        self.oarea, self.tri_id, self.tri_cnt, self.doarea = (t.cpu().numpy() for t in out[3:7])
        B, H, W = self.depth.shape
        self.image = image_state(out[9], B, H, W)
        self.face_list = face_list(out[8], self.num_rendered)


def backward(mod, fwd, dL_dcolor, dL_ddepth):
    """The reference's backward on its own forward's buffers -> the six gradients (numpy), in util.GRAD_NAMES order."""
    import torch
    o = fwd.out
    g = mod.render_backward_cuda(o[0], *fwd.dargs, dL_dcolor, dL_ddepth, o[7], o[8], o[9], o[3], o[4], _with_slack(o[5]), o[6])
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in g]


def _with_slack(tri_cnt):
    """``tri_cnt`` (B, H, W) as a view of a larger allocation.  The reference's backward reads oarea_buffer_tri_cnt[b][y][x]
    from EVERY thread of a 16 x 16 tile before it looks whether the thread has a pixel (backward.cu:156): where H or W is no
    multiple of 16 the threads right of the patch read other pixels' counts and those below the last view's patch read up to
    (H16 - H) * W + (W16 - W) entries past the end of the tensor.  The value is never used (such a thread is ``done``), so the
    gradients are defined, but the load itself must stay inside memory the process owns: the view's storage has that many
    zero entries behind it."""
    import torch
    B, H, W = tri_cnt.shape
    n = B * H * W
    slack = (-(-H // 16) * 16 - H) * W + (-(-W // 16) * 16 - W)
    buf = torch.zeros(n + slack, dtype=tri_cnt.dtype, device=tri_cnt.device)
    buf[:n] = tri_cnt.reshape(-1)
    return buf[:n].view(B, H, W)


def generate_layers(mod, dargs):
    """The reference's generate_render_layers_cuda -> render_layers, render_layers_cnt (numpy).  Only at image sizes that are
    multiples of the 16 x 16 tile: its first-intersection kernel stores first_face / first_tet = -1 from every thread of a tile
    before it looks whether the thread has a pixel, so at other sizes threads right of the image overwrite other pixels' entries
    and threads below it store past the end of the buffer."""
    import torch
    W, H = int(dargs[0]), int(dargs[1])
    if W % 16 or H % 16:
        raise ValueError("the reference's layer generator is only defined where width and height are multiples of 16")
    _defined(dargs[3], dargs[8], dargs[9], np.zeros((dargs[8].shape[0], 2), np.float32), W, H)
    layers, cnt = mod.generate_render_layers_cuda(*dargs)
    torch.cuda.synchronize()
    return layers.cpu().numpy(), cnt.cpu().numpy()


def races_in_binning(faces, verts_ndc, verts_image, patch_min, W, H):
    """(B, F) bool: the faces over which the reference's binning races.  Its counting kernel drops a face whose ndc z lies wholly
    below -1 or above 1 before it looks at the face's tile rectangle; its emitting kernel does not repeat that test and writes
    one entry per tile of the rectangle from the slot where the NEXT faces' entries begin (the dropped face owns no slots),
    with a depth key that was never stored.  Where such a face has a non-empty rectangle, the tile lists depend on which
    thread stores last (and the stores of the last faces can pass the end of the list): the reference defines nothing there."""
    fc = np.asarray(faces).astype(np.int64)
    z = np.asarray(verts_ndc, np.float32)[:, fc, 2]                           # (B,F,3)
    dropped = (z.max(-1) < -1.0) | (z.min(-1) > 1.0)
    p = np.asarray(verts_image, np.float32)[:, fc] - np.asarray(patch_min, np.float32)[:, None, None, :]   # (B,F,3,2)
    grid = np.array([(W + 15) // 16, (H + 15) // 16], np.float64)
    with np.errstate(all="ignore"):
        lo = np.clip(np.floor(p.min(2).astype(np.float64) / 16.0), 0, grid)
        hi = np.clip(np.ceil(p.max(2).astype(np.float64) / 16.0), 0, grid)
    return dropped & ((hi - lo) > 0).all(-1)


TILE_LIMIT = 2.0 ** 31 - 128.0            # the largest float32 below 2^31: up to it (and down to its negative) float -> int is defined


def undefined_tile_rects(verts_ndc, verts_image, patch_min):
    """None, or why the reference's binning defines nothing for these arguments.  Both of its kernels compute a face's tile
    rectangle as (int)floorf((coordinate - patch_min) / 16) (auxiliary.h:75-82); the conversion is only defined for a finite
    quotient inside int's range.  The depth key and the z test read verts_ndc z, which must be finite to order anything."""
    ndc, img = np.asarray(verts_ndc, np.float32), np.asarray(verts_image, np.float32)
    if not np.isfinite(ndc[..., 2]).all():
        return "verts_ndc holds a non-finite z"
    if not np.isfinite(img).all():
        return "verts_image holds a non-finite coordinate"
    with np.errstate(all="ignore"):
        q = (img - np.asarray(patch_min, np.float32)[:, None, :]) / np.float32(16.0)
    if img.size and float(np.abs(q).max()) > TILE_LIMIT:
        return "a tile coordinate of verts_image lies outside int's range"
    return None


def _defined(faces, verts_ndc, verts_image, patch_min, W, H):
    t = [x.detach().cpu().numpy() if hasattr(x, "detach") else x for x in (faces, verts_ndc, verts_image, patch_min)]
    why = undefined_tile_rects(t[1], t[2], t[3])
    if why:
        raise ValueError("the reference's binning is not defined here: " + why)
    n = int(races_in_binning(*t, W, H).sum())
    if n:
        raise ValueError(f"the reference's binning races over {n} faces of this scene (dropped by the z test, with a tile rectangle)")


# ---- acceptance of gradients -----------------------------------------------------------------------------------------------
def accept_gradients(ref, others, f64, tol):
    """Hold ``others`` = {who: {tensor: array}} to the reference's gradients ``ref`` = {tensor: array}, tensor by tensor.

    A tensor passes where every one of ``others`` lies within ``tol`` (relative L-inf of the tensor's maximum) of the reference.
    The reference sums with float atomics in no fixed order, so where a tensor misses that, ``f64()`` -> {tensor: float64
    array} is computed (once) and the REFERENCE is measured against it: if the reference itself lies farther than ``tol``
    from float64, the bound becomes twice the reference's own distance (two independent fp32 summation orders may each be as
    far off as the reference is) and everyone is measured against float64; if the reference is within ``tol`` of float64
    there is no relief.  The widened bound never comes from ``others``.

    -> (figures {tensor: dict(vs_ref {who: e}[, ref_vs_f64, bound, vs_f64 {who: e}])}, widened [tensor], failures [(tensor,
    who, figure, bound)])."""
    from util import rel_linf
    figures, widened, failures = {}, [], []
    g64 = None
    for nm, r in ref.items():
        d = {who: rel_linf(o[nm], r) for who, o in others.items()}
        fig = figures[nm] = dict(vs_ref=d)
        if max(d.values()) <= tol:
            continue
        if g64 is None:
            g64 = f64()
        e_ref = fig["ref_vs_f64"] = rel_linf(r, g64[nm])
        if e_ref > tol:
            bound = fig["bound"] = 2.0 * e_ref
            e = fig["vs_f64"] = {who: rel_linf(o[nm], g64[nm]) for who, o in others.items()}
            widened.append(nm)
            failures += [(nm, who, v, bound) for who, v in e.items() if v > bound]
        else:
            failures += [(nm, who, v, tol) for who, v in d.items() if v > tol]
    return figures, widened, failures


def describe(figures):
    """One line per call: each tensor's worst figure against the reference, and what a widened tensor was measured with."""
    out = []
    for nm, f in figures.items():
        s = f"{nm} " + "/".join(f"{v:.2e}" for v in f["vs_ref"].values())
        if "ref_vs_f64" in f:
            s += f" [reference vs float64 {f['ref_vs_f64']:.2e}"
            if "bound" in f:
                s += f", WIDENED to {f['bound']:.2e}, vs float64 " + "/".join(f"{v:.2e}" for v in f["vs_f64"].values())
            s += "]"
        out.append(s)
    return ", ".join(out)
