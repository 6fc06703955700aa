"""``_C``-compatible shim over libdm2_hip.so (include/dm2_hip.h).

Exposes the three functions of the reference's pybind module
``dmesh2_renderer._C`` (ext.cpp:5-9) with identical positional arguments and
tuple returns:

    render_forward_cuda(...21 args...)  -> 10-tuple   (render.cu:28-195)
    render_backward_cuda(...31 args...) -> 6-tuple    (render.cu:198-373)
    generate_render_layers_cuda(...13 args...) -> 2-tuple (render.cu:378-476)

and the consumer of those layers the reference does not have (LayeredRenderer.render):

    composite_layers_cuda(...10 args...) -> 4-tuple, composite_layers_backward_cuda(...13 args...) -> 4-tuple

and the per-pixel nearest hits of any triangle mesh (Renderer.rasterize):

    rasterize_layers_cuda(...10 args...) -> 4-tuple, rasterize_layers_backward_cuda(...7 args...) -> dL/dverts
    (both with ``overlap=True``: the faces that overlap the pixel's square, a 5-tuple with the ``inside`` mask)

and the attribute images of such hits (Renderer.interpolate):

    interpolate_cuda(render_layers, bary, attr, attr_faces) -> out,
    interpolate_backward_cuda(...those 4..., grad_out, need_attr, need_bary) -> (dL/dattr, dL/dbary)

and a texture sampled at such an image of UVs (Renderer.texture):

    texture_cuda(uv, tex, render_layers, filter_mode, boundary_mode) -> out,
    texture_backward_cuda(...those 5..., grad_out, need_tex, need_uv) -> (dL/dtex, dL/duv)

and a cube map looked up by such an image of directions (Renderer.texture's boundary_mode="cube"):

    texture_cube_cuda(dirs, tex, render_layers, filter_mode) -> out,
    texture_cube_backward_cuda(...those 4..., grad_out, need_tex, need_dirs) -> (dL/dtex, dL/ddirs)

and a voxel grid looked up by such an image of positions (Renderer.texture3d):

    texture_volume_cuda(xyz, grid, render_layers, filter_mode, boundary_mode) -> out,
    texture_volume_backward_cuda(...those 5..., grad_out, need_grid, need_xyz) -> (dL/dgrid, dL/dxyz)

and a multiresolution hash encoding looked up by such positions (Renderer.hash_grid):

    hash_grid_resolutions(num_levels, base_resolution, growth) -> [R_0, ..., R_{NL-1}],
    hash_grid_cuda(xyz, table, render_layers, base_resolution, growth, filter_mode, boundary_mode) -> out,
    hash_grid_backward_cuda(...those 7..., grad_out, need_table, need_xyz) -> (dL/dtable, dL/dxyz)

and its mip-mapped filter (Renderer.bary_derivatives, Renderer.texture_mipmaps, texture's "linear-mipmap-linear"):

    bary_derivatives_cuda(render_layers, verts, faces, ray_cam) -> (dbary_dx, dbary_dy),
    texture_mipmaps_cuda(tex, max_mip_level) -> mip,  texture_mipmaps_backward_cuda(tex, max_mip_level, grad_mip) -> dL/dtex,
    texture_mip_cuda(uv, uv_da, tex, mip, render_layers, boundary_mode, max_mip_level) -> out,
    texture_mip_backward_cuda(...those 7..., grad_out, need_tex, need_mip, need_uv) -> (dL/dtex, dL/dmip, dL/duv)

and the cube's mip chain at a level of detail per slot (texture's "linear-mipmap-linear" with "cube" and mip_level):

    texture_cube_mip_cuda(dirs, level, tex, mip, render_layers, max_mip_level) -> out,
    texture_cube_mip_backward_cuda(...those 6..., grad_out, need_tex, need_mip, need_dirs, need_level)
        -> (dL/dtex, dL/dmip, dL/ddirs, dL/dlevel)

and the GGX prefilter that turns a cube's box chain into a roughness chain (Renderer.cube_prefilter):

    cube_prefilter_cuda(chain, N, max_mip_level) -> filtered chain,  cube_prefilter_transpose_cuda(grad, N, max_mip_level) -> xbar

and such per-slot values blended into an image (Renderer.composite; not composite_layers_cuda, which shades by itself):

    composite_cuda(values, alpha, render_layers, background) -> (out, acc, final_T, n_contrib),
    composite_backward_cuda(...those 4..., n_contrib, grad_out, grad_acc, need_values, need_alpha) -> (dL/dvalues, dL/dalpha)

and the analytic pixel coverage of listed faces, the anti-aliasing factor of such a blend's alpha (Renderer.coverage):

    coverage_cuda(render_layers, verts_image, faces, temperature) -> cov,
    coverage_backward_cuda(...those 4..., grad_cov) -> dL/dverts_image

and what feeds a cube-map lookup (Renderer.vertex_normals, Renderer.shading_vectors):

    vertex_normals_cuda(verts, faces, offsets, corners, normalize) -> (normals, len),
    vertex_normals_backward_cuda(...those 5..., normals, len, grad_normals) -> dL/dverts,
    shading_vectors_cuda(render_layers, t, normals, image_ray_o, image_ray_d) -> (position, view[, normal, reflection]),
    shading_vectors_backward_cuda(...those 5..., g_position, g_normal, g_reflection, need_t, need_normals) -> (dL/dt, dL/dnormals)

Under the ``alpha_output`` side channel render_forward_cuda appends the alpha (coverage) image; the two backwards take
its gradient as the keyword ``dL_dout_alpha``.  Under ``face_weights_output`` render_forward_cuda and composite_layers_cuda
append the per-face blend weights (B,F), behind everything else they return; they have no gradient.

PyTorch is used only as the owner of device memory and of the current stream;
every computation happens in the HIP library.  There is NO fallback: if the
library is missing, or tensors are not on a ROCm device, a RuntimeError is
raised.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Callable, NamedTuple, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DM2_HIP_LIB") or os.path.join(_HERE, "csrc", "libdm2_hip.so")   # env override: A/B builds
_lib = None
_lock = threading.Lock()

DM2_FLAG_CORRECTED_DV = 1
DM2_FLAG_LEGACY_KERNELS = 2
DM2_FLAG_NO_BACKWARD = 4
DM2_FLAG_ANALYTIC_RAYS = 8
DM2_FLAG_AA_GRAD_TO_VERTS = 16
DM2_FLAG_TABLES_FROM_IMAGE = 32
DM2_FLAG_NO_PAIR_POOL = 64
SCRATCH_FACE, SCRATCH_IMAGE, SCRATCH_BINNING, SCRATCH_LAYER_IMAGE, SCRATCH_LAYER_TETS, SCRATCH_PAIR_POOL, SCRATCH_TIE_QUEUE = range(7)
# what a forward left for its backward (include/dm2_hip.h DM2_FWD_*)
FWD_UNKNOWN, FWD_NONE, FWD_MASKS, FWD_POOL, FWD_POINT = 0, 1, 2, 3, 4
ABI_VERSION = 8

# opt-in flags applied to every call (tests use this for the corrected-gradient mode)
_flags = 0
_bin_hint: dict = {}      # (device, B, W, H, F) -> bytes of binning scratch (+ pair pool) that held the last forward of that shape; under _lock

_vp, _i32, _i64, _sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t


class RenderDesc(ctypes.Structure):
    _fields_ = [
        ("B", _i32), ("P", _i32), ("F", _i32), ("W", _i32), ("H", _i32), ("K", _i32),
        ("aa_temperature", ctypes.c_float), ("flags", _i32), ("full_W", _i32), ("full_H", _i32),
        ("background", _vp), ("patch_min", _vp), ("verts", _vp), ("faces", _vp), ("verts_color", _vp),
        ("faces_opacity", _vp), ("verts_ndc", _vp), ("verts_image", _vp), ("faces_intense", _vp),
        ("aa_face_verts", _vp), ("aa_face_edges", _vp), ("aa_face_edges_iszero", _vp),
        ("aa_face_edges_recip", _vp), ("aa_face_edges_normal", _vp), ("aa_face_edges_normal_c", _vp),
        ("image_ray_o", _vp), ("image_ray_d", _vp), ("ray_cam", _vp),
    ]


class PrepDesc(ctypes.Structure):
    _fields_ = [
        ("B", _i32), ("P", _i32), ("F", _i32), ("W", _i32), ("H", _i32),
        ("verts", _vp), ("faces", _vp), ("mv", _vp), ("proj", _vp),
        ("verts_ndc", _vp), ("verts_image", _vp), ("aa_face_verts", _vp), ("aa_face_edges", _vp),
        ("aa_face_edges_iszero", _vp), ("aa_face_edges_recip", _vp), ("aa_face_edges_normal", _vp),
        ("aa_face_edges_normal_c", _vp),
    ]


class LayersDesc(ctypes.Structure):
    _fields_ = [
        ("B", _i32), ("P", _i32), ("F", _i32), ("T", _i32), ("W", _i32), ("H", _i32), ("L", _i32), ("flags", _i32),
        ("verts", _vp), ("faces", _vp), ("tets", _vp), ("face_tets", _vp), ("tet_faces", _vp),
        ("face_existence", _vp), ("verts_ndc", _vp), ("verts_image", _vp), ("image_ray_o", _vp), ("image_ray_d", _vp),
        ("ray_cam", _vp),
    ]


class LayerCompositeDesc(ctypes.Structure):
    _fields_ = [
        ("B", _i32), ("P", _i32), ("F", _i32), ("W", _i32), ("H", _i32), ("L", _i32), ("flags", _i32),
        ("render_layers", _vp), ("verts", _vp), ("faces", _vp), ("verts_color", _vp), ("faces_opacity", _vp),
        ("faces_intense", _vp), ("verts_ndc", _vp), ("background", _vp), ("image_ray_o", _vp), ("image_ray_d", _vp),
        ("ray_cam", _vp),
    ]


class Window(ctypes.Structure):
    _fields_ = [("patch_min", _vp), ("full_W", _i32), ("full_H", _i32)]


EXPORTS = {
    # name: (restype, argtypes)
    "dm2_abi_version": (ctypes.c_int, []),
    "dm2_last_error": (ctypes.c_char_p, []),
    "dm2_scratch_bytes": (_sz, [ctypes.c_int, _i64, _i64]),
    "dm2_forward_plan": (ctypes.c_int, [ctypes.POINTER(RenderDesc), _vp, _sz, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "dm2_forward_run": (ctypes.c_int, [ctypes.POINTER(RenderDesc), _i64, _i64, _i64, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp,
                                       ctypes.POINTER(_i32)]),
    "dm2_forward": (ctypes.c_int, [ctypes.POINTER(RenderDesc), _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp,
                                   ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i32)]),
    "dm2_forward_alpha": (ctypes.c_int, [ctypes.POINTER(RenderDesc), _vp, _sz, _vp, _vp]),
    "dm2_backward": (ctypes.c_int, [ctypes.POINTER(RenderDesc), _i64, _i32, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dm2_layers_plan": (ctypes.c_int, [ctypes.POINTER(LayersDesc), ctypes.POINTER(Window), _vp, _sz, _vp, ctypes.POINTER(_i64),
                                       ctypes.POINTER(_i64)]),
    "dm2_layers_run": (ctypes.c_int, [ctypes.POINTER(LayersDesc), ctypes.POINTER(Window), _i64, _i64, _vp, _sz, _vp, _sz, _vp, _sz,
                                      _vp, _sz, _vp, _vp, _vp]),
    "dm2_rasterize_run": (ctypes.c_int, [ctypes.POINTER(LayersDesc), ctypes.POINTER(Window), _i64, _i64, _vp, _sz, _vp, _sz, _vp, _sz,
                                         _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "dm2_rasterize_backward": (ctypes.c_int, [ctypes.POINTER(LayersDesc), ctypes.POINTER(Window), _vp, _vp, _vp, _vp, _i32, _vp]),
    "dm2_interpolate": (ctypes.c_int, [_i32] * 8 + [_vp] * 6),
    "dm2_interpolate_backward": (ctypes.c_int, [_i32] * 8 + [_vp] * 8),
    "dm2_texture": (ctypes.c_int, [_i32] * 10 + [_vp] * 5),
    "dm2_texture_backward": (ctypes.c_int, [_i32] * 10 + [_vp] * 7),
    "dm2_texture_cube": (ctypes.c_int, [_i32] * 8 + [_vp] * 5),
    "dm2_texture_cube_backward": (ctypes.c_int, [_i32] * 8 + [_vp] * 7),
    "dm2_texture_volume": (ctypes.c_int, [_i32] * 9 + [_vp] * 5),
    "dm2_texture_volume_backward": (ctypes.c_int, [_i32] * 9 + [_vp] * 7),
    "dm2_hash_grid": (ctypes.c_int, [_i32] * 11 + [_vp] * 5),
    "dm2_hash_grid_backward": (ctypes.c_int, [_i32] * 11 + [_vp] * 7),
    "dm2_vertex_normals_scratch_bytes": (_sz, [_i32] * 3),
    "dm2_vertex_normals": (ctypes.c_int, [_i32] * 3 + [_vp] * 5 + [_sz] + [_vp] * 3),
    "dm2_vertex_normals_backward": (ctypes.c_int, [_i32] * 3 + [_vp] * 8 + [_sz] + [_vp] * 2),
    "dm2_shading_vectors_window": (ctypes.c_int, [_i32] * 5 + [ctypes.POINTER(Window)] + [_vp] * 11),
    "dm2_shading_vectors_backward_window": (ctypes.c_int, [_i32] * 5 + [ctypes.POINTER(Window)] + [_vp] * 12),
    "dm2_bary_derivatives_window": (ctypes.c_int, [_i32] * 6 + [ctypes.POINTER(Window)] + [_vp] * 7),
    "dm2_texture_mipmaps": (ctypes.c_int, [_i32] * 5 + [_vp] * 3),
    "dm2_texture_mipmaps_backward": (ctypes.c_int, [_i32] * 5 + [_vp] * 3),
    "dm2_texture_mip": (ctypes.c_int, [_i32] * 10 + [_vp] * 7),
    "dm2_texture_mip_backward": (ctypes.c_int, [_i32] * 10 + [_vp] * 10),
    "dm2_texture_cube_mip": (ctypes.c_int, [_i32] * 8 + [_vp] * 7),
    "dm2_texture_cube_mip_backward": (ctypes.c_int, [_i32] * 8 + [_vp] * 10),
    "dm2_cube_prefilter": (ctypes.c_int, [_i32] * 4 + [_vp] * 3),
    "dm2_cube_prefilter_backward": (ctypes.c_int, [_i32] * 4 + [_vp] * 3),
    "dm2_composite": (ctypes.c_int, [_i32] * 7 + [_vp] * 9),
    "dm2_composite_backward": (ctypes.c_int, [_i32] * 7 + [_vp] * 10),
    "dm2_coverage": (ctypes.c_int, [_i32] * 6 + [ctypes.c_float, ctypes.POINTER(Window)] + [_vp] * 6),
    "dm2_coverage_backward": (ctypes.c_int, [_i32] * 6 + [ctypes.c_float, ctypes.POINTER(Window)] + [_vp] * 6),
    "dm2_layers_composite": (ctypes.c_int, [ctypes.POINTER(LayerCompositeDesc), ctypes.POINTER(Window), _vp, _vp, _vp, _vp, _vp, _vp]),
    "dm2_layers_composite_backward": (ctypes.c_int, [ctypes.POINTER(LayerCompositeDesc), ctypes.POINTER(Window), _vp, _vp, _vp, _vp,
                                                     _vp, _vp, _vp, _vp, _vp]),
    "dm2_prepare_faces": (ctypes.c_int, [ctypes.POINTER(PrepDesc), _vp]),
    "dm2_prepare_faces_backward": (ctypes.c_int, [ctypes.POINTER(PrepDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "dm2_prepare_faces_camera_scratch_bytes": (_sz, [_i32, _i32]),
    "dm2_prepare_faces_backward_camera": (ctypes.c_int, [ctypes.POINTER(PrepDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dm2_exchange_mark": (ctypes.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _sz, _vp, _vp, _vp]),
    "dm2_exchange_pack": (ctypes.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dm2_exchange_unpack": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp]),
    "dm2_debug_aa_overlap": (ctypes.c_int, [ctypes.c_int, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dm2_debug_fetch": (ctypes.c_int, [ctypes.c_int, _i64, _i64, _i64, _vp, _sz, _vp, _vp]),
    "dm2_profile_enable": (None, [ctypes.c_int]),
    "dm2_profile_read": (ctypes.c_int, [ctypes.POINTER(ctypes.c_float), ctypes.c_int]),
    "dm2_debug_stamps": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int]),
}

STAGE_NAMES = ["preprocess_scan", "bin_scatter", "tile_sort", "tile_ranges", "forward_composite", "backward_composite", "backward_ties"]


def profile_enable(on: bool):
    load_library().dm2_profile_enable(1 if on else 0)


def profile_read():
    """Per-stage milliseconds of the calling thread's most recent forward/backward (see dm2_profile_read)."""
    buf = (ctypes.c_float * len(STAGE_NAMES))()
    n = load_library().dm2_profile_read(buf, len(STAGE_NAMES))
    return {STAGE_NAMES[i]: float(buf[i]) for i in range(n)}


def load_library(path: str | None = None):
    """dlopen libdm2_hip.so and bind every symbol include/dm2_hip.h declares."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise RuntimeError(
                f"dmesh2_renderer_amd: native library not found at {p}; build it with "
                f"`python -c 'import __graft_entry__ as g; g.build()'` or `make -C dmesh2_renderer_amd/csrc` "
                f"(there is no CPU fallback)")
        lib = ctypes.CDLL(p)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(lib, name)       # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if lib.dm2_abi_version() != ABI_VERSION:
            raise RuntimeError("dmesh2_renderer_amd: ABI version mismatch")
        if path is None:
            _lib = lib
        return lib


def set_flags(flags: int):
    """Set opt-in behaviour flags (DM2_FLAG_*) for subsequent calls; returns the old value."""
    global _flags
    old, _flags = _flags, int(flags)
    return old


def _err(lib, what):
    msg = lib.dm2_last_error()
    return RuntimeError(f"{what}: {msg.decode() if msg else 'unknown error'}")


def _bad(cond, msg):
    if cond:
        raise RuntimeError(msg)


def _require_gpu(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(
                "dmesh2_renderer_amd: all tensors must live on a ROCm GPU (got a CPU tensor); "
                "this build has no CPU path -- the CPU restatement under oracle/ is test infrastructure only")
    dev = tensors[0].device
    for t in tensors:
        if t.device != dev:
            raise RuntimeError("dmesh2_renderer_amd: tensors are on different devices")
    return dev


def _c(t, dtype):
    if t.dtype != dtype:
        raise RuntimeError(f"expected dtype {dtype}, got {t.dtype}")      # packed_accessor64<T> throws likewise
    return t.contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _bytes(dev, n):
    return torch.empty((max(int(n), 0),), dtype=torch.uint8, device=dev)


def _check_render_shapes(background, patch_min, verts, faces, verts_color, faces_opacity, verts_ndc, verts_image,
                         faces_intense, aa_v, aa_e, aa_z, aa_r, aa_n, aa_c, ray_o, ray_d, temp, K):
    # messages of render.cu:62-118
    _bad(background.dim() != 1 or background.size(0) != 3, "background must have dimensions (3,)")
    _bad(patch_min.dim() != 2 or patch_min.size(1) != 2, "patch_min must have dimensions (B, 2)")
    _bad(verts.dim() != 2 or verts.size(1) != 3, "verts must have dimensions (P, 3)")
    _bad(faces.dim() != 2 or faces.size(1) != 3, "faces must have dimensions (F, 3)")
    _bad(verts_color.dim() != 2 or verts_color.size(1) != 3, "vert color must have dimensions (P, 3)")
    _bad(faces_opacity.dim() != 1 or faces_opacity.size(0) != faces.size(0), "face opacity must have dimensions (F,)")
    _bad(verts_ndc.dim() != 3 or verts_ndc.size(2) != 3, "verts_ndc must have dimensions (B, P, 3)")
    _bad(verts_image.dim() != 3 or verts_image.size(2) != 2, "verts_image must have dimensions (B, P, 2)")
    _bad(faces_intense.dim() != 2 or faces_intense.size(1) != faces.size(0), "faces_intense must have dimensions (B, F,)")
    for t, nm in ((aa_v, "aa_face_verts"), (aa_e, "aa_face_edges"), (aa_z, "aa_face_edges_iszero"),
                  (aa_r, "aa_face_edges_recip"), (aa_n, "aa_face_edges_normal")):
        _bad(t.dim() != 4 or t.size(2) != 3 or t.size(3) != 2, f"{nm} must have dimensions (B, F, 3, 2)")
    _bad(aa_c.dim() != 3 or aa_c.size(2) != 3, "aa_face_edges_normal_c must have dimensions (B, F, 3)")
    _bad(ray_o.dim() != 4 or ray_o.size(3) != 3, "image_ray_o must have dimensions (B, H, W, 3)")
    _bad(ray_d.dim() != 4 or ray_d.size(3) != 3, "image_ray_d must have dimensions (B, H, W, 3)")
    _bad(temp < 0 or temp > 1, "aa_temperature must be in the range [0, 1]")
    _bad(K < 0, "len_oarea_buffer must be non-negative")


def _make_desc(args, keep):
    (background, patch_min, pw, ph, verts, faces, verts_color, faces_opacity, verts_ndc, verts_image, faces_intense,
     temp, aa_v, aa_e, aa_z, aa_r, aa_n, aa_c, K, ray_o, ray_d) = args
    temp = float(temp); K = int(K); pw = int(pw); ph = int(ph)
    _check_render_shapes(background, patch_min, verts, faces, verts_color, faces_opacity, verts_ndc, verts_image,
                         faces_intense, aa_v, aa_e, aa_z, aa_r, aa_n, aa_c, ray_o, ray_d, temp, K)
    dev = _require_gpu(background, patch_min, verts, faces, verts_color, faces_opacity, verts_ndc, verts_image,
                       faces_intense, aa_v, aa_e, aa_z, aa_r, aa_n, aa_c, ray_o, ray_d)
    f32, i32 = torch.float32, torch.int32
    B, P, F = verts_ndc.size(0), verts.size(0), faces.size(0)
    # sizes the kernels index with (the reference's accessors would fault on a mismatch)
    def need(t, shape, nm):
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{nm} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    need(patch_min, (B, 2), "patch_min"); need(verts_color, (P, 3), "verts_color"); need(verts_ndc, (B, P, 3), "verts_ndc")
    need(verts_image, (B, P, 2), "verts_image"); need(faces_intense, (B, F), "faces_intense")
    from_image = bool(getattr(_tls, "tables_from_image", False))
    if not from_image:
        for t, nm in ((aa_v, "aa_face_verts"), (aa_e, "aa_face_edges"), (aa_z, "aa_face_edges_iszero"),
                      (aa_r, "aa_face_edges_recip"), (aa_n, "aa_face_edges_normal")):
            need(t, (B, F, 3, 2), nm)
        need(aa_c, (B, F, 3), "aa_face_edges_normal_c")
    ana = _analytic(B, dev)
    if ana is None:
        need(ray_o, (B, ph, pw, 3), "image_ray_o"); need(ray_d, (B, ph, pw, 3), "image_ray_d")
    if temp == 0.0:
        K = 0                                                     # render.cu:141-142
    ts = dict(
        background=_c(background, f32), patch_min=_c(patch_min, i32), verts=_c(verts, f32), faces=_c(faces, i32),
        verts_color=_c(verts_color, f32), faces_opacity=_c(faces_opacity, f32), verts_ndc=_c(verts_ndc, f32),
        verts_image=_c(verts_image, f32), faces_intense=_c(faces_intense, f32), aa_face_verts=_c(aa_v, f32),
        aa_face_edges=_c(aa_e, f32), aa_face_edges_iszero=_c(aa_z, torch.bool), aa_face_edges_recip=_c(aa_r, f32),
        aa_face_edges_normal=_c(aa_n, f32), aa_face_edges_normal_c=_c(aa_c, f32), image_ray_o=_c(ray_o, f32),
        image_ray_d=_c(ray_d, f32))
    keep.append(ts)
    d = RenderDesc()
    d.B, d.P, d.F, d.W, d.H, d.K = B, P, F, pw, ph, K
    d.aa_temperature = temp
    d.flags = _flags
    for k, t in ts.items():
        setattr(d, k, t.data_ptr() if t.numel() > 0 else None)
    if from_image:
        d.flags |= DM2_FLAG_TABLES_FROM_IMAGE
        for k in ("aa_face_verts", "aa_face_edges", "aa_face_edges_iszero", "aa_face_edges_recip", "aa_face_edges_normal", "aa_face_edges_normal_c"):
            setattr(d, k, None)
    if ana is not None:
        cam, fw, fh = ana
        keep.append(cam)
        d.flags |= DM2_FLAG_ANALYTIC_RAYS
        d.ray_cam, d.full_W, d.full_H = cam.data_ptr(), fw, fh
        d.image_ray_o = d.image_ray_d = None
    return d, dev, (B, P, F, pw, ph, K)


def _tiles(B, W, H):
    return B * ((W + 15) // 16) * ((H + 15) // 16)


_tls = threading.local()


class _SideChannel:
    """Base of the side channels below: a per-thread value that the ``*_cuda`` calls read from ``_tls`` (attribute ``_slot``,
    ``_off`` outside every block).  Entering sets it, leaving restores what was there before, so blocks nest."""
    _slot, _off = "", False

    def __init__(self, on=True):
        self.val = bool(on)

    def __enter__(self):
        self.old = getattr(_tls, self._slot, self._off)
        setattr(_tls, self._slot, self.val)

    def __exit__(self, *exc):
        setattr(_tls, self._slot, self.old)


class forward_only(_SideChannel):
    """``with _C.forward_only(True): _C.render_forward_cuda(...)`` -- no backward will follow this forward (RenderFunction
    sets it when no input requires a gradient, e.g. under ``torch.no_grad()``): the blend masks a backward would use are
    not written.  A side channel on purpose: the function keeps the reference's exact 21-argument signature."""
    _slot = "forward_only"


class analytic_rays(_SideChannel):
    """``with _C.analytic_rays(ray_cam, width, height): _C.render_forward_cuda(...)`` (and the matching backward /
    generate_render_layers call): the primary rays are computed per pixel from ``ray_cam`` (B,32) float32 = inv(mv) then
    inv(proj) of each rendered view, row-major, for an image of (width, height) -- the operation order of the reference's
    ``Renderer._init_rays`` -- and the ``image_ray_o`` / ``image_ray_d`` arguments are placeholders of shape (B,0,0,3)
    that are never read.  A side channel like ``forward_only``: the 21 / 31 / 13-argument
    signatures stay the reference's."""
    _slot, _off = "analytic", None

    def __init__(self, ray_cam, width, height):
        self.val = None if ray_cam is None else (ray_cam, int(width), int(height))


class window(_SideChannel):
    """``with _C.window(patch_min, full_width, full_height): _C.rasterize_layers_cuda(...)`` (and generate_render_layers /
    coverage / composite_layers, and their backwards): the call works on a window of the frame.  ``patch_min`` (B,2) int32 on
    the GPU = the (x, y) origin of each view's window in its (full_width, full_height) frame; the call's width / height, its
    ray tensors and every (B,H,W,...) tensor are then the window's (include/dm2_hip.h: dm2_window), which the entry
    points are handed.  That the windows lie inside the frame is the caller's check (Renderer does it, with one read-back).  None:
    no window, the calls as they are without one.  A side channel like ``analytic_rays``: the signatures stay as they are."""
    _slot, _off = "window", None

    def __init__(self, patch_min, full_width=0, full_height=0):
        self.val = None if patch_min is None else (patch_min, int(full_width), int(full_height))


def _window(B, W, H, dev, keep):
    """The thread's window for a call of B views and a W x H window on ``dev`` -> ctypes Window, or None (no window)."""
    w = getattr(_tls, "window", None)
    if w is None:
        return None
    pm, fw, fh = w
    if pm.dtype != torch.int32 or tuple(pm.shape) != (B, 2) or pm.device != dev:
        raise RuntimeError(f"window: patch_min must be int32 (B, 2) on {dev}, got {pm.dtype} {tuple(pm.shape)} on {pm.device}")
    if W > fw or H > fh:
        raise RuntimeError(f"window: a {W} x {H} window does not fit a {fw} x {fh} frame")
    pm = pm.contiguous()
    keep.append(pm)
    win = Window()
    win.patch_min, win.full_W, win.full_H = (pm.data_ptr() if pm.numel() > 0 else None), fw, fh
    return win


def _win(win):
    """``_window``'s result as the ``const dm2_window*`` argument: NULL without a window."""
    return None if win is None else ctypes.byref(win)


def _frame_size(width, height):
    """The size analytic rays must have been declared for: the frame of the thread's window, or the call's own width / height."""
    w = getattr(_tls, "window", None)
    return (w[1], w[2]) if w is not None else (width, height)


class aa_grad_to_verts(_SideChannel):
    """``with _C.aa_grad_to_verts(True): _C.render_backward_cuda(...)`` -- the sixth gradient is not dL/d(aa_face_verts)
    (B,F,3,2) but that gradient already scattered to the vertices the corners belong to, (B,P,2): the gradient of
    ``verts_image`` through the reordered copy (DM2_FLAG_AA_GRAD_TO_VERTS).  For a caller that owns the host prep as well
    (Renderer with the fused prep).  A side channel like ``forward_only``: the 31-argument signature stays the reference's."""
    _slot = "aa_to_verts"


class tables_from_image(_SideChannel):
    """``with _C.tables_from_image(True): _C.render_forward_cuda(...)`` (and the matching backward): the six ``aa_*`` arguments
    are placeholders (any tensors of the right rank, e.g. ``(B, 0, 3, 2)``) that are never read -- the plan builds the tables
    per (view, face) from ``verts_image[faces]`` in registers, exactly as ``Triangles`` would (DM2_FLAG_TABLES_FROM_IMAGE).  For a
    caller that owns the host prep (Renderer with the fused prep); the AA-corner gradients then come back per vertex
    (``aa_grad_to_verts``).  A side channel like ``forward_only``: the 21 / 31-argument signatures stay the reference's."""
    _slot = "tables_from_image"


class alpha_output(_SideChannel):
    """``with _C.alpha_output(True): _C.render_forward_cuda(...)`` -- the forward returns an 11-tuple: the reference's ten
    outputs, then the alpha (coverage) image (B,H,W) float32 = 1 - T, the T the colour multiplied the background by (zeros
    when nothing is rendered; dm2_forward_alpha).  Its gradient goes to ``render_backward_cuda(..., dL_dout_alpha=g)``.  Also
    read by ``LayeredCompositeFunction``.  A side channel like ``forward_only``: the 21-argument signature stays the
    reference's."""
    _slot = "alpha_output"


class face_weights_output(_SideChannel):
    """``with _C.face_weights_output(True): _C.render_forward_cuda(...)`` -- the forward appends face_weights (B,F) float32
    behind everything else it returns (behind alpha under ``alpha_output``): per view and face the sum, over the pixels of
    the patch, of alpha * T of each of the face's blends -- the factor its colour gets in C += c alpha T
    (dm2_forward's out_face_weights).  Float atomics: the last bits may vary from run to run.  No gradient.  Also read by
    ``composite_layers_cuda`` (dm2_layers_composite's out_face_weights) and ``LayeredCompositeFunction``."""
    _slot = "face_weights_output"


class forward_mode(_SideChannel):
    """``with _C.forward_mode(mode): _C.render_backward_cuda(...)`` -- tells the backward what the forward of this frame left
    for it (FWD_NONE / FWD_MASKS / FWD_POOL, as ``_C.last_forward_mode()`` reported right after that forward), so that it
    launches exactly one composite kernel.  Without it the binning buffer's own note is used when the very tensor object the
    forward returned comes back; otherwise (FWD_UNKNOWN) every candidate kernel is launched and all but one return at once.
    A side channel like ``forward_only``: the 31-argument signature stays the reference's."""
    _slot, _off = "fwd_mode", None

    def __init__(self, mode):
        self.val = mode


def last_forward_mode():
    """FWD_* of the calling thread's most recent render_forward_cuda."""
    return getattr(_tls, "last_fwd_mode", FWD_UNKNOWN)


def last_pair_bound():
    """The pair bound the plan of the calling thread's most recent render_forward_cuda counted: the (pixel, face) pairs its
    composite may enumerate, which sized the pair pool of the binning buffer (0 when nothing was planned)."""
    return getattr(_tls, "last_pair_bound", 0)


def _pool_budget(N, R):
    """Pairs the shim is willing to give pool room to (4 B each in the binning buffer + 16 B each of backward scratch, 8 GB at
    the cap): a frame whose plan counts more candidate pairs than this -- hundreds of faces over every pixel of a large image,
    thousands of screen-filling faces -- keeps blend masks only and its backward re-clips (DM2_FWD_MASKS)."""
    return min(max(256 * N, 16 * R, 1 << 24), 400_000_000)


def _analytic(B, dev):
    a = getattr(_tls, "analytic", None)
    if a is None:
        return None
    cam, w, h = a
    if cam.dtype != torch.float32 or tuple(cam.shape) != (B, 32) or cam.device != dev:
        raise RuntimeError(f"analytic_rays: ray_cam must be float32 (B, 32) on {dev}, got {cam.dtype} {tuple(cam.shape)} on {cam.device}")
    return cam.contiguous(), w, h


def _analytic_onto(d, ana, width, height, keep, mismatch):
    """Analytic rays (``_analytic``'s result, or None: nothing happens) onto a layers / composite descriptor of a
    width x height call: the flag, the cameras, no ray tensors.  ``mismatch``: the caller's words for a frame size that
    differs from the one the rays were declared for."""
    if ana is None:
        return
    _bad((ana[1], ana[2]) != _frame_size(width, height), mismatch)
    keep.append(ana[0])
    d.flags |= DM2_FLAG_ANALYTIC_RAYS
    d.ray_cam = ana[0].data_ptr()
    d.image_ray_o = d.image_ray_d = None


def _layers_plan(lib, d, win, dev, st, what):
    """The plan step of a dm2_layers_desc (generate, rasterize): face and image scratch, dm2_layers_plan, then the binning
    scratch its count asks for -> (num_rendered, longest tile list, face_buf, bin_buf, img_buf)."""
    N, Tn = d.B * d.H * d.W, _tiles(d.B, d.W, d.H)
    face_buf = _bytes(dev, lib.dm2_scratch_bytes(SCRATCH_FACE, d.B * d.F, 2 * Tn))
    img_buf = _bytes(dev, lib.dm2_scratch_bytes(SCRATCH_LAYER_IMAGE, N, Tn))
    nr, longest = _i64(0), _i64(0)
    if lib.dm2_layers_plan(ctypes.byref(d), _win(win), _ptr(face_buf), face_buf.numel(), st, ctypes.byref(nr), ctypes.byref(longest)):
        raise _err(lib, f"{what} (plan)")
    R = int(nr.value)
    return R, int(longest.value), face_buf, _bytes(dev, lib.dm2_scratch_bytes(SCRATCH_BINNING, R, Tn)), img_buf


def render_forward_cuda(*args):
    """(num_rendered, color, depth, oarea, tri_id, tri_cnt, doarea, face_buffer, binning_buffer, img_buffer).

    The four AA-record tensors and three byte buffers are opaque to callers
    (reference __init__.py:103-109,160-166).  This implementation recomputes AA
    overlaps in the backward pass, so ``oarea``/``tri_id``/``doarea`` are empty
    (B,H,W,0[,3,2]) placeholders; ``tri_cnt`` (B,H,W) holds the number of
    records the reference would have taken (min(#overlaps visited, K)).
    """
    if len(args) != 21:
        raise TypeError(f"render_forward_cuda() takes 21 positional arguments ({len(args)} given)")
    lib = load_library()
    keep: list = []
    d, dev, (B, P, F, W, H, K) = _make_desc(args, keep)
    if getattr(_tls, "forward_only", False):
        d.flags |= DM2_FLAG_NO_BACKWARD
    if getattr(_tls, "aa_to_verts", False):
        d.flags |= DM2_FLAG_AA_GRAD_TO_VERTS          # the packed records note the CCW reorder for the backward
    want_alpha = bool(getattr(_tls, "alpha_output", False))
    want_weights = bool(getattr(_tls, "face_weights_output", False))
    with torch.cuda.device(dev):
        st = _stream(dev)
        f32, i32 = torch.float32, torch.int32
        weights = torch.zeros((B, F), dtype=f32, device=dev) if want_weights else None   # (accumulated by the composite)
        color = torch.empty((B, H, W, 3), dtype=f32, device=dev)
        depth = torch.empty((B, H, W), dtype=f32, device=dev)
        oarea = torch.empty((B, H, W, 0), dtype=f32, device=dev)
        tri_id = torch.empty((B, H, W, 0), dtype=i32, device=dev)
        doarea = torch.empty((B, H, W, 0, 3, 2), dtype=f32, device=dev)
        N, Tn, BF = B * H * W, _tiles(B, W, H), B * F
        if P == 0 or BF == 0 or N == 0:
            # render.cu:149: nothing is rendered; outputs are the zero-initialised images
            color.zero_(); depth.zero_()
            tri_cnt = torch.zeros((B, H, W), dtype=i32, device=dev)
            e = _bytes(dev, 0)
            _tls.last_pair_bound = 0
            out = (0, color, depth, oarea, tri_id, tri_cnt, doarea, e, _bytes(dev, 0), _bytes(dev, 0))
            if want_alpha:
                out += (torch.zeros((B, H, W), dtype=f32, device=dev),)
            return out + (weights,) if want_weights else out
        tri_cnt = torch.empty((B, H, W), dtype=i32, device=dev)
        face_buf = _bytes(dev, lib.dm2_scratch_bytes(SCRATCH_FACE, BF, 2 * Tn + 1))
        img_buf = _bytes(dev, lib.dm2_scratch_bytes(SCRATCH_IMAGE, N, Tn))
        nr, longest, pairs, mode = _i64(0), _i64(0), _i64(0), _i32(0)
        # the binning scratch (+ pair pool) is sized from the last call on this device (+ 25 %): when it fits -- every step of
        # a training loop but the first -- plan and run are one C call and the GPU does not wait for Python in between
        key = (dev.index, B, W, H, F)
        with _lock:
            hint = _bin_hint.get(key, 0)
        if _pool_budget(N, 0) <= 0:
            d.flags |= DM2_FLAG_NO_PAIR_POOL
        bin_buf = _bytes(dev, hint)
        rc = lib.dm2_forward(ctypes.byref(d), _ptr(face_buf), face_buf.numel(), _ptr(bin_buf), bin_buf.numel(), _ptr(img_buf),
                             img_buf.numel(), _ptr(color), _ptr(depth), _ptr(tri_cnt), _ptr(weights), st, ctypes.byref(nr),
                             ctypes.byref(longest), ctypes.byref(pairs), ctypes.byref(mode))
        if rc not in (0, 2):
            raise _err(lib, "render_forward_cuda")
        R = int(nr.value)
        wants_pool = d.aa_temperature > 0.0 and not (d.flags & (DM2_FLAG_NO_BACKWARD | DM2_FLAG_LEGACY_KERNELS | DM2_FLAG_NO_PAIR_POOL))
        over = wants_pool and int(pairs.value) > _pool_budget(N, R)
        pool = lib.dm2_scratch_bytes(SCRATCH_PAIR_POOL, int(pairs.value), 0) if wants_pool and not over else 0
        need = lib.dm2_scratch_bytes(SCRATCH_BINNING, R, Tn) + pool
        if rc == 2 or (over and int(mode.value) == FWD_POOL):
            # (over budget although last frame's buffer happened to have room: rendered again with masks only, so that the
            # backward's tie scratch stays within the budget too)
            if over:
                d.flags |= DM2_FLAG_NO_PAIR_POOL
            bin_buf = _bytes(dev, need + need // 4)
            if want_weights:
                weights.zero_()                       # (the over-budget case composited once already: the sums start again)
            if lib.dm2_forward_run(ctypes.byref(d), R, int(longest.value), int(pairs.value), _ptr(face_buf), face_buf.numel(),
                                   _ptr(bin_buf), bin_buf.numel(), _ptr(img_buf), img_buf.numel(), _ptr(color), _ptr(depth),
                                   _ptr(tri_cnt), _ptr(weights), st, ctypes.byref(mode)):
                raise _err(lib, "render_forward_cuda (run)")
        with _lock:
            hint = _bin_hint.get(key, 0)
            if need > hint or 2 * (need + need // 4) < hint:
                if len(_bin_hint) > 64:
                    _bin_hint.clear()
                _bin_hint[key] = need + need // 4
        if want_alpha:
            alpha = torch.empty((B, H, W), dtype=f32, device=dev)
            if lib.dm2_forward_alpha(ctypes.byref(d), _ptr(img_buf), img_buf.numel(), _ptr(alpha), st):
                raise _err(lib, "render_forward_cuda (alpha)")
    _tls.last_fwd_mode = int(mode.value)
    _tls.last_pair_bound = int(pairs.value)
    bin_buf._dm2_fwd_mode = int(mode.value)       # (survives only as long as this very tensor object is passed around)
    out = (R, color, depth, oarea, tri_id, tri_cnt, doarea, face_buf, bin_buf, img_buf)
    if want_alpha:
        out += (alpha,)
    return out + (weights,) if want_weights else out


def packed_grads(P, F, B, aa_to_verts, device):
    """Six zero gradients in the order render_backward_cuda returns them, as views of ONE packed fp32 buffer (attribute
    ``_dm2_packed`` on the first).  Physical order: the gradients of the LEAVES first ([dverts | dverts_color | dfaces_opacity |
    dfaces_intense], one contiguous span for a multi-GPU caller), then the two intermediates of the host prep (dverts_ndc,
    daa_face_verts: (B,P,2) when ``aa_to_verts``, else (B,F,3,2)).  The one statement of that layout: a rank without a band
    (sharding.BandShardedOp) and the CPU test double build theirs here, so every rank takes the same path through the
    collectives."""
    sizes = [P * 3, P * 3, F, B * F, B * P * 3, B * P * 2 if aa_to_verts else B * F * 6]
    packed = torch.zeros((sum(sizes),), dtype=torch.float32, device=device)
    parts = torch.split(packed, sizes)
    g_verts = parts[0].view(P, 3); g_color = parts[1].view(P, 3); g_opac = parts[2].view(F)
    g_int = parts[3].view(B, F); g_ndc = parts[4].view(B, P, 3)
    g_aa = parts[5].view(B, P, 2) if aa_to_verts else parts[5].view(B, F, 3, 2)
    g_verts._dm2_packed = packed
    return g_verts, g_color, g_opac, g_ndc, g_int, g_aa


def render_backward_cuda(*args, dL_dout_alpha=None):
    """-> (dL_dverts, dL_dverts_color, dL_dfaces_opacity, dL_dverts_ndc, dL_dfaces_intense, dL_daa_face_verts).

    The six gradients are views of ONE packed fp32 buffer (attribute
    ``_dm2_packed`` on the first tensor) so that a multi-GPU caller can sum
    them with a single RCCL all-reduce (dmesh2_renderer_amd.sharding).
    dL_dout_alpha (B,H,W) or None: the gradient of the alpha image of ``alpha_output`` (dm2_backward's dL_dout_alpha).
    """
    if len(args) != 31:
        raise TypeError(f"render_backward_cuda() takes 31 positional arguments ({len(args)} given)")
    lib = load_library()
    num_rendered = int(args[0])
    fwd_args = args[1:22]
    dL_dcolor, dL_ddepth = args[22], args[23]
    face_buf, bin_buf, img_buf = args[24], args[25], args[26]
    keep: list = []
    d, dev, (B, P, F, W, H, K) = _make_desc(fwd_args, keep)
    _require_gpu(dL_dcolor, dL_ddepth)
    f32 = torch.float32
    to_verts = bool(getattr(_tls, "aa_to_verts", False))
    if to_verts:
        d.flags |= DM2_FLAG_AA_GRAD_TO_VERTS
    g_verts, g_color, g_opac, g_ndc, g_int, g_aa = packed_grads(P, F, B, to_verts, dev)      # render.cu:313-318 zeros_like x6
    if F != 0 and P != 0 and num_rendered > 0 and B * H * W > 0:
        if tuple(dL_dcolor.shape) != (B, H, W, 3) or tuple(dL_ddepth.shape) != (B, H, W):
            raise RuntimeError("dL_dout_color / dL_dout_depth must have dimensions (B, H, W, 3) / (B, H, W)")
        dc = _c(dL_dcolor, f32); dd = _c(dL_ddepth, f32)
        da = None
        if dL_dout_alpha is not None:
            if tuple(dL_dout_alpha.shape) != (B, H, W):
                raise RuntimeError("dL_dout_alpha must have dimensions (B, H, W)")
            _require_gpu(dL_dcolor, dL_dout_alpha)
            da = _c(dL_dout_alpha, f32)
        mode = getattr(_tls, "fwd_mode", None)
        if mode is None:
            mode = getattr(bin_buf, "_dm2_fwd_mode", FWD_UNKNOWN)
        with torch.cuda.device(dev):
            # scratch of this call: the queue of the pairs whose AA Jacobian the exact clipper has to supply -- room for one entry
            # per pair of the binning buffer's pool part (written only for the 1-5 % that are ties)
            tie_buf = None
            if mode not in (FWD_MASKS, FWD_NONE) and d.aa_temperature > 0.0 and not (d.flags & DM2_FLAG_LEGACY_KERNELS):
                pool_pairs = max(0, bin_buf.numel() - lib.dm2_scratch_bytes(SCRATCH_BINNING, num_rendered, _tiles(B, W, H))) // 4
                if pool_pairs > 0:
                    tie_buf = _bytes(dev, lib.dm2_scratch_bytes(SCRATCH_TIE_QUEUE, pool_pairs, 0))
            if lib.dm2_backward(ctypes.byref(d), num_rendered, int(mode), _ptr(dc), _ptr(dd), _ptr(da),
                                _ptr(face_buf), face_buf.numel(), _ptr(bin_buf), bin_buf.numel(), _ptr(img_buf), img_buf.numel(),
                                _ptr(tie_buf), tie_buf.numel() if tie_buf is not None else 0,
                                _ptr(g_verts), _ptr(g_color), _ptr(g_opac), _ptr(g_ndc), _ptr(g_int), _ptr(g_aa), _stream(dev)):
                raise _err(lib, "render_backward_cuda")
    return g_verts, g_color, g_opac, g_ndc, g_int, g_aa


def generate_render_layers_cuda(width, height, verts, faces, tets, face_tets, tet_faces, face_existence,
                                verts_ndc, verts_image, image_ray_o, image_ray_d, num_layers):
    """-> (render_layers (B,H,W,L) int32, -1 = empty; render_layers_cnt (B,H,W) int32)."""
    lib = load_library()
    # messages of render.cu:397-429
    _bad(verts.dim() != 2 or verts.size(1) != 3, "verts must have dimensions (P, 3)")
    _bad(faces.dim() != 2 or faces.size(1) != 3, "faces must have dimensions (F, 3)")
    _bad(tets.dim() != 2 or tets.size(1) != 4, "tets must have dimensions (T, 4)")
    _bad(face_tets.dim() != 2 or face_tets.size(1) != 2, "face_tets must have dimensions (F, 2)")
    _bad(tet_faces.dim() != 2 or tet_faces.size(1) != 4, "tet_faces must have dimensions (T, 4)")
    _bad(face_existence.dim() != 1 or face_existence.size(0) != faces.size(0), "face_existence must have dimensions (F,)")
    _bad(verts_ndc.dim() != 3 or verts_ndc.size(2) != 3, "verts_ndc must have dimensions (B, P, 3)")
    _bad(verts_image.dim() != 3 or verts_image.size(2) != 2, "verts_image must have dimensions (B, P, 2)")
    _bad(image_ray_o.dim() != 4 or image_ray_o.size(3) != 3, "image_ray_o must have dimensions (B, H, W, 3)")
    _bad(image_ray_d.dim() != 4 or image_ray_d.size(3) != 3, "image_ray_d must have dimensions (B, H, W, 3)")
    num_layers = int(num_layers); width = int(width); height = int(height)
    _bad(num_layers < 0, "num_layers must be non-negative")
    dev = _require_gpu(verts, faces, tets, face_tets, tet_faces, face_existence, verts_ndc, verts_image, image_ray_o, image_ray_d)
    f32, i32 = torch.float32, torch.int32
    B, P, F, T = verts_ndc.size(0), verts.size(0), faces.size(0), tets.size(0)
    _bad(tuple(face_tets.shape) != (F, 2), "face_tets must have dimensions (F, 2)")
    _bad(tuple(tet_faces.shape) != (T, 4), "tet_faces must have dimensions (T, 4)")
    _bad(tuple(verts_ndc.shape) != (B, P, 3) or tuple(verts_image.shape) != (B, P, 2), "verts_ndc/verts_image shape mismatch")
    ana = _analytic(B, dev)
    keep: list = []
    win = _window(B, width, height, dev, keep)           # (then width / height and the rays are the window's)
    _bad(ana is None and (tuple(image_ray_o.shape) != (B, height, width, 3) or tuple(image_ray_d.shape) != (B, height, width, 3)),
        "image_ray_o/image_ray_d must have dimensions (B, H, W, 3)")
    ts = dict(verts=_c(verts, f32), faces=_c(faces, i32), tets=_c(tets, i32), face_tets=_c(face_tets, i32),
              tet_faces=_c(tet_faces, i32), face_existence=_c(face_existence, i32), verts_ndc=_c(verts_ndc, f32),
              verts_image=_c(verts_image, f32), image_ray_o=_c(image_ray_o, f32), image_ray_d=_c(image_ray_d, f32))
    d = LayersDesc()
    d.B, d.P, d.F, d.T, d.W, d.H, d.L, d.flags = B, P, F, T, width, height, num_layers, _flags
    for k, t in ts.items():
        setattr(d, k, t.data_ptr() if t.numel() > 0 else None)
    _analytic_onto(d, ana, width, height, keep, "analytic_rays: the image size differs from generate_render_layers_cuda's width / height")
    with torch.cuda.device(dev):
        st = _stream(dev)
        cnt = torch.zeros((B, height, width), dtype=i32, device=dev)              # render.cu:437
        layers = torch.full((B, height, width, num_layers), -1, dtype=i32, device=dev)   # render.cu:438
        if B * height * width == 0 or F == 0 or T == 0:
            # no pixels, no face to hit, or no tet to enter (a walk starts in a tet: without tets every first_tet is -1, and
            # face_tets may still name tets that are not there): the filled defaults, nothing is launched
            return layers, cnt
        R, longest, face_buf, bin_buf, img_buf = _layers_plan(lib, d, win, dev, st, "generate_render_layers_cuda")
        tet_buf = _bytes(dev, lib.dm2_scratch_bytes(SCRATCH_LAYER_TETS, T, 0))
        if lib.dm2_layers_run(ctypes.byref(d), _win(win), R, longest, _ptr(face_buf), face_buf.numel(), _ptr(bin_buf), bin_buf.numel(),
                              _ptr(img_buf), img_buf.numel(), _ptr(tet_buf), tet_buf.numel(), _ptr(layers), _ptr(cnt), st):
            raise _err(lib, "generate_render_layers_cuda (run)")
    generate_render_layers_cuda.last_debug = (R, face_buf, bin_buf, img_buf)      # kept for tests
    return layers, cnt


def _rasterize_desc(width, height, B, verts, faces, image_ray_o, image_ray_d, num_layers, keep, face_existence=None,
                    verts_ndc=None, verts_image=None):
    """Checks (in the style of generate_render_layers_cuda) + the dm2_layers_desc of a rasterize call (T = 0: no tets); under
    ``window``, width / height and the rays are the window's.  The backward passes no face_existence / verts_ndc / verts_image:
    it reads neither."""
    _bad(verts.dim() != 2 or verts.size(1) != 3, "verts must have dimensions (P, 3)")
    _bad(faces.dim() != 2 or faces.size(1) != 3, "faces must have dimensions (F, 3)")
    _bad(face_existence is not None and (face_existence.dim() != 1 or face_existence.size(0) != faces.size(0)),
        "face_existence must have dimensions (F,)")
    _bad(verts_ndc is not None and (verts_ndc.dim() != 3 or verts_ndc.size(2) != 3), "verts_ndc must have dimensions (B, P, 3)")
    _bad(verts_image is not None and (verts_image.dim() != 3 or verts_image.size(2) != 2), "verts_image must have dimensions (B, P, 2)")
    _bad(image_ray_o.dim() != 4 or image_ray_o.size(3) != 3, "image_ray_o must have dimensions (B, H, W, 3)")
    _bad(image_ray_d.dim() != 4 or image_ray_d.size(3) != 3, "image_ray_d must have dimensions (B, H, W, 3)")
    num_layers = int(num_layers); width = int(width); height = int(height)
    _bad(num_layers < 0, "num_layers must be non-negative")
    tensors = [t for t in (verts, faces, face_existence, verts_ndc, verts_image, image_ray_o, image_ray_d) if t is not None]
    dev = _require_gpu(*tensors)
    f32, i32 = torch.float32, torch.int32
    P, F = verts.size(0), faces.size(0)
    _bad((verts_ndc is not None and tuple(verts_ndc.shape) != (B, P, 3)) or (verts_image is not None and tuple(verts_image.shape) != (B, P, 2)),
        "verts_ndc/verts_image shape mismatch")
    ana = _analytic(B, dev)
    _bad(ana is None and (tuple(image_ray_o.shape) != (B, height, width, 3) or tuple(image_ray_d.shape) != (B, height, width, 3)),
        "image_ray_o/image_ray_d must have dimensions (B, H, W, 3)")
    ts = dict(verts=_c(verts, f32), faces=_c(faces, i32), image_ray_o=_c(image_ray_o, f32), image_ray_d=_c(image_ray_d, f32))
    for k, x, dt in (("face_existence", face_existence, i32), ("verts_ndc", verts_ndc, f32), ("verts_image", verts_image, f32)):
        if x is not None:
            ts[k] = _c(x, dt)
    keep += list(ts.values())
    d = LayersDesc()
    d.B, d.P, d.F, d.T, d.W, d.H, d.L, d.flags = B, P, F, 0, width, height, num_layers, _flags
    for k, t in ts.items():
        setattr(d, k, t.data_ptr() if t.numel() > 0 else None)
    _analytic_onto(d, ana, width, height, keep, "analytic_rays: the image size differs from the rasterize call's width / height")
    return d, dev


def rasterize_layers_cuda(width, height, verts, faces, face_existence, verts_ndc, verts_image, image_ray_o, image_ray_d,
                          num_layers, overlap=False):
    """The first ``num_layers`` faces each pixel's ray hits, in (t, face id) order (include/dm2_hip.h: dm2_rasterize_run).

    verts (P,3), faces (F,3) int32, face_existence (F) int32 or None (every face exists), verts_ndc (B,P,3), verts_image
    (B,P,2) of the full frame (the plan's bins and depth cull), image_ray_o / image_ray_d (B,H,W,3) (placeholders under
    ``analytic_rays``) -> (render_layers (B,H,W,L) int32, -1 = empty; render_layers_cnt (B,H,W) int32; bary (B,H,W,L,3) float32
    = (1 - u - v, u, v); t (B,H,W,L) float32), -1 in every empty slot.

    ``overlap=True`` (dm2_rasterize_run's overlap mode): the faces that overlap the pixel's square and whose plane the ray meets
    in front, with clamped barycentrics -> the same four and inside (B,H,W,L) bool, true where the ray hits the face itself."""
    lib = load_library()
    keep: list = []
    if verts_ndc is None or verts_ndc.dim() != 3 or verts_image is None:
        raise RuntimeError("verts_ndc / verts_image must have dimensions (B, P, 3) / (B, P, 2)")
    d, dev = _rasterize_desc(width, height, verts_ndc.size(0), verts, faces, image_ray_o, image_ray_d, num_layers, keep,
                             face_existence=face_existence, verts_ndc=verts_ndc, verts_image=verts_image)
    win = _window(d.B, d.W, d.H, dev, keep)
    B, F, H, W, L = d.B, d.F, d.H, d.W, d.L
    f32, i32 = torch.float32, torch.int32
    if B * H * W == 0 or L == 0 or F == 0:
        # nothing to walk: every slot empty (the kernels would write the same)
        out = (torch.full((B, H, W, L), -1, dtype=i32, device=dev), torch.zeros((B, H, W), dtype=i32, device=dev),
               torch.full((B, H, W, L, 3), -1.0, dtype=f32, device=dev), torch.full((B, H, W, L), -1.0, dtype=f32, device=dev))
        return out + (torch.zeros((B, H, W, L), dtype=torch.bool, device=dev),) if overlap else out
    layers = torch.empty((B, H, W, L), dtype=i32, device=dev)            # (every slot written by the kernel)
    inside = torch.empty((B, H, W, L), dtype=torch.uint8, device=dev) if overlap else None
    cnt = torch.empty((B, H, W), dtype=i32, device=dev)
    bary = torch.empty((B, H, W, L, 3), dtype=f32, device=dev)
    t = torch.empty((B, H, W, L), dtype=f32, device=dev)
    with torch.cuda.device(dev):
        st = _stream(dev)
        R, longest, face_buf, bin_buf, img_buf = _layers_plan(lib, d, win, dev, st, "rasterize_layers_cuda")
        if lib.dm2_rasterize_run(ctypes.byref(d), _win(win), R, longest, _ptr(face_buf), face_buf.numel(), _ptr(bin_buf), bin_buf.numel(),
                                 _ptr(img_buf), img_buf.numel(), _ptr(layers), _ptr(cnt), _ptr(bary), _ptr(t), 1 if overlap else 0,
                                 _ptr(inside), st):
            raise _err(lib, "rasterize_layers_cuda (run)")
    if overlap:
        return layers, cnt, bary, t, inside.view(torch.bool)       # (the kernel writes 0 or 1)
    return layers, cnt, bary, t


def rasterize_layers_backward_cuda(render_layers, verts, faces, image_ray_o, image_ray_d, dL_dbary, dL_dt, overlap=False):
    """Gradient of rasterize_layers_cuda's bary and t w.r.t. verts (dm2_rasterize_backward): render_layers (B,H,W,L) as the
    forward returned them, the forward's verts / faces / rays, dL_dbary (B,H,W,L,3) and dL_dt (B,H,W,L), either may be None
    -> dL_dverts (P,3).  Nothing flows through the rays or through which faces are listed.  ``overlap=True``: the lists are the
    overlap mode's (dm2_rasterize_backward with overlap set: the clamp is recomputed and chained through)."""
    lib = load_library()
    if render_layers.dim() != 4:
        raise RuntimeError("render_layers must have dimensions (B, H, W, L)")
    B, H, W, L = (int(x) for x in render_layers.shape)
    keep: list = []
    d, dev = _rasterize_desc(W, H, B, verts, faces, image_ray_o, image_ray_d, L, keep)
    win = _window(B, W, H, dev, keep)
    f32 = torch.float32
    checks = []
    if dL_dbary is not None:
        checks.append((dL_dbary, (B, H, W, L, 3), "dL_dbary"))
    if dL_dt is not None:
        checks.append((dL_dt, (B, H, W, L), "dL_dt"))
    for x, shape, nm in checks:
        if tuple(x.shape) != shape:
            raise RuntimeError(f"{nm} must have dimensions {shape}, got {tuple(x.shape)}")
    _require_gpu(verts, render_layers, *[x for x, _, _ in checks])
    rl = _c(render_layers, torch.int32)
    gb = _c(dL_dbary, f32) if dL_dbary is not None else None
    gt = _c(dL_dt, f32) if dL_dt is not None else None
    dverts = torch.zeros((d.P, 3), dtype=f32, device=dev)
    if B * H * W * L == 0 or d.F == 0 or (gb is None and gt is None):
        return dverts
    with torch.cuda.device(dev):
        if lib.dm2_rasterize_backward(ctypes.byref(d), _win(win), _ptr(rl), _ptr(gb), _ptr(gt), _ptr(dverts), 1 if overlap else 0,
                                      _stream(dev)):
            raise _err(lib, "rasterize_layers_backward_cuda")
    return dverts


def _interpolate_args(render_layers, bary, attr, attr_faces, grad_out=None):
    """Checks of an interpolate call -> (sizes (B, H, W, L, F, N, C, view_tables), contiguous tensors, device)."""
    _bad(render_layers.dim() != 4, "render_layers must have dimensions (B, H, W, L)")
    B, H, W, L = (int(x) for x in render_layers.shape)
    _bad(tuple(bary.shape) != (B, H, W, L, 3), f"bary must have dimensions {(B, H, W, L, 3)}, got {tuple(bary.shape)}")
    _bad(attr.dim() not in (2, 3), "attr must have dimensions (N, C) or (B, N, C)")
    _bad(attr.dim() == 3 and attr.size(0) != B, f"attr must have dimensions (N, C) or ({B}, N, C), got {tuple(attr.shape)}")
    _bad(attr.size(-1) < 1, "attr must have at least one channel")
    _bad(attr_faces.dim() != 2 or attr_faces.size(1) != 3, "attr_faces must have dimensions (F, 3)")
    N, C, F = int(attr.size(-2)), int(attr.size(-1)), int(attr_faces.size(0))
    _bad(grad_out is not None and tuple(grad_out.shape) != (B, H, W, L, C),
        f"grad_out must have dimensions {(B, H, W, L, C)}, got {tuple(grad_out.shape) if grad_out is not None else None}")
    dev = _require_gpu(*[t for t in (render_layers, bary, attr, attr_faces, grad_out) if t is not None])
    f32, i32 = torch.float32, torch.int32
    named = (("render_layers", render_layers, i32), ("bary", bary, f32), ("attr", attr, f32), ("attr_faces", attr_faces, i32),
             ("grad_out", grad_out, f32))
    ts = []
    for name, t, dt in named:
        _bad(t is not None and t.dtype != dt, f"{name}: expected dtype {dt}, got {t.dtype if t is not None else None}")
        ts.append(None if t is None else t.contiguous())
    return (B, H, W, L, F, N, C, 1 if attr.dim() == 3 else 0), ts, dev


def interpolate_cuda(render_layers, bary, attr, attr_faces):
    """Attribute images from per-slot face ids and barycentrics (include/dm2_hip.h: dm2_interpolate).

    render_layers (B,H,W,L) int32, bary (B,H,W,L,3) float32, attr (N,C) or (B,N,C) float32, attr_faces (F,3) int32 rows of attr
    -> out (B,H,W,L,C) float32 = (bary0 attr[v0] + bary1 attr[v1]) + bary2 attr[v2]; 0 where the id is outside [0, F) or a
    row of attr_faces[id] outside [0, N)."""
    lib = load_library()
    sizes, (rl, bc, at, af, _), dev = _interpolate_args(render_layers, bary, attr, attr_faces)
    B, H, W, L, F, N, C, _ = sizes
    if B * H * W * L == 0 or F == 0 or N == 0:
        return torch.zeros((B, H, W, L, C), dtype=torch.float32, device=dev)      # every slot empty: no launch
    out = torch.empty((B, H, W, L, C), dtype=torch.float32, device=dev)         # (every element written by the kernel)
    with torch.cuda.device(dev):
        if lib.dm2_interpolate(*sizes, _ptr(rl), _ptr(bc), _ptr(at), _ptr(af), _ptr(out), _stream(dev)):
            raise _err(lib, "interpolate_cuda")
    return out


def interpolate_backward_cuda(render_layers, bary, attr, attr_faces, grad_out, need_attr, need_bary):
    """Gradients of interpolate_cuda (dm2_interpolate_backward) -> (dL_dattr of attr's shape or None, dL_dbary (B,H,W,L,3) or
    None): only what ``need_attr`` / ``need_bary`` ask for is computed."""
    lib = load_library()
    sizes, (rl, bc, at, af, go), dev = _interpolate_args(render_layers, bary, attr, attr_faces, grad_out)
    B, H, W, L, F, N, C, _ = sizes
    f32 = torch.float32
    dattr = torch.zeros(tuple(attr.shape), dtype=f32, device=dev) if need_attr else None
    if not (need_attr or need_bary):
        return None, None
    if B * H * W * L == 0 or F == 0 or N == 0:
        return dattr, torch.zeros((B, H, W, L, 3), dtype=f32, device=dev) if need_bary else None
    dbary = torch.empty((B, H, W, L, 3), dtype=f32, device=dev) if need_bary else None
    with torch.cuda.device(dev):
        if lib.dm2_interpolate_backward(*sizes, _ptr(rl), _ptr(bc), _ptr(at), _ptr(af), _ptr(go), _ptr(dattr), _ptr(dbary),
                                        _stream(dev)):
            raise _err(lib, "interpolate_backward_cuda")
    return dattr, dbary


# -- the per-slot lookup ops: a coordinate per slot (B,H,W,L,k), a table and optional render_layers -> out (B,H,W,L,C); the
#    backward returns the table's gradient (summed into) and the coordinate's (fully written).  Each op is one ``_Lookup``
#    record and two thin wrappers; ``_lookup_args`` / ``_lookup_forward`` / ``_lookup_backward`` do the rest. -------------------
TEX_FILTERS = {"nearest": 0, "linear": 1}        # include/dm2_hip.h DM2_TEX_FILTER_*
TEX_BOUNDARIES = {"wrap": 0, "clamp": 1}         # DM2_TEX_BOUNDARY_*
# ABI 7's words for a volume's boundary, then OR-ed into dm2_texture_cube's filter.  Nothing here sends them and the library
# refuses them as unknown filters.  The name stays because ABI 7's test modules read it when they are imported: without it
# that suite cannot even be collected against this library, with it exactly the tests of the retired encoding fail.
TEX_VOLUME_BOUNDARIES = {"clamp": 0x100, "wrap": 0x200}
HASH_GRID_FEATURES = (1, 2, 4, 8)
HASH_GRID_MAX_LEVELS, HASH_GRID_MAX_RESOLUTION = 32, 2 ** 20
HASH_GRID_LOG2_ROWS = (4, 24)


def _hash_grid_q(growth):
    """growth -> q = 16 growth, an integer in 17..32 (ValueError otherwise)."""
    q = float(growth) * 16.0
    if not (17.0 <= q <= 32.0 and q == int(q)):                          # (NaN fails the first test)
        raise ValueError(f"growth must be a multiple of 1/16 from 1.0625 to 2, got {growth!r}")
    return int(q)


def hash_grid_resolutions(num_levels, base_resolution=16, growth=1.5):
    """The level resolutions of a hash grid (include/dm2_hip.h, dm2_hash_grid): R_0 = base_resolution,
    R_{l+1} = (R_l * q) >> 4 with q = 16 growth.  ValueError for a growth that is no multiple of 1/16 in [1.0625, 2], fewer than
    1 or more than 32 levels, a base resolution below 1 or a finest level above 2^20."""
    q = _hash_grid_q(growth)
    num_levels, base_resolution = int(num_levels), int(base_resolution)
    if not 1 <= num_levels <= HASH_GRID_MAX_LEVELS:
        raise ValueError(f"num_levels must be in 1..{HASH_GRID_MAX_LEVELS}, got {num_levels}")
    if base_resolution < 1:
        raise ValueError(f"base_resolution must be at least 1, got {base_resolution}")
    res = [base_resolution]
    while len(res) < num_levels:
        res.append((res[-1] * q) >> 4)
    if res[-1] > HASH_GRID_MAX_RESOLUTION:
        raise ValueError(f"the finest level's resolution must not exceed 2^20, got {res[-1]}")
    return res


# The table checks of each op: (table, B, filter_mode, boundary_mode, ...) -> (the ABI words behind (B, H, W, L), C).
def _texture_table(tex, B, filter_mode, boundary_mode):
    _bad(tex.dim() not in (3, 4), "tex must have dimensions (Ht, Wt, C) or (B, Ht, Wt, C)")
    _bad(tex.dim() == 4 and tex.size(0) != B, f"tex must have dimensions (Ht, Wt, C) or ({B}, Ht, Wt, C), got {tuple(tex.shape)}")
    Ht, Wt, C = (int(x) for x in tex.shape[-3:])
    _bad(Ht < 1 or Wt < 1, "tex must have at least one row and one column")
    _bad(C < 1, "tex must have at least one channel")
    _bad(Ht * Wt >= 2 ** 31, "tex: Ht * Wt must be below 2^31")
    return (Ht, Wt, C, 1 if tex.dim() == 4 else 0, TEX_FILTERS[filter_mode], TEX_BOUNDARIES[boundary_mode]), C


def _cube_table(tex, B, filter_mode, boundary_mode):
    _bad(tex.dim() not in (4, 5), "tex must have dimensions (6, N, N, C) or (B, 6, N, N, C)")
    _bad(tex.dim() == 5 and tex.size(0) != B, f"tex must have dimensions (6, N, N, C) or ({B}, 6, N, N, C), got {tuple(tex.shape)}")
    six, Nr, N, C = (int(x) for x in tex.shape[-4:])
    _bad(six != 6, f"tex must have six faces, (6, N, N, C) or ({B}, 6, N, N, C), got {tuple(tex.shape)}")
    _bad(Nr != N, f"tex must have square faces, got {tuple(tex.shape)}")
    _bad(N < 1, "tex must have at least one row and one column per face")
    _bad(C < 1, "tex must have at least one channel")
    _bad(6 * N * N >= 2 ** 31, "tex: 6 * N * N must be below 2^31")
    return (N, C, 1 if tex.dim() == 5 else 0, TEX_FILTERS[filter_mode]), C


def _volume_table(grid, B, filter_mode, boundary_mode):
    _bad(grid.dim() not in (4, 5), "grid must have dimensions (N, N, N, C) or (B, N, N, N, C)")
    _bad(grid.dim() == 5 and grid.size(0) != B, f"grid must have dimensions (N, N, N, C) or ({B}, N, N, N, C), got {tuple(grid.shape)}")
    Nk, Nj, N, C = (int(x) for x in grid.shape[-4:])
    _bad(Nk != N or Nj != N, f"grid must be a cube, (N, N, N, C) or ({B}, N, N, N, C), got {tuple(grid.shape)}")
    _bad(N < 1, "grid must have at least one voxel")
    _bad(C < 1, "grid must have at least one channel")
    _bad(N * N * N >= 2 ** 31, "grid: N * N * N must be below 2^31")
    return (N, C, 1 if grid.dim() == 5 else 0, TEX_FILTERS[filter_mode], TEX_BOUNDARIES[boundary_mode]), C


def _hash_grid_table(table, B, filter_mode, boundary_mode, base_resolution, growth):
    _bad(table.dim() != 3, f"table must have dimensions (NL, T, F), got {tuple(table.shape)}")
    NL, T, F = (int(x) for x in table.shape)
    _bad(not 1 <= NL <= HASH_GRID_MAX_LEVELS, f"table must have 1..{HASH_GRID_MAX_LEVELS} levels, got {NL}")
    log2T = T.bit_length() - 1
    _bad(T < 1 or (1 << log2T) != T or not HASH_GRID_LOG2_ROWS[0] <= log2T <= HASH_GRID_LOG2_ROWS[1],
         f"table must have a power of two from 2^4 to 2^24 rows per level, got {T}")
    _bad(F not in HASH_GRID_FEATURES, f"table must have 1, 2, 4 or 8 features per row, got {F}")
    _bad(NL * T * F >= 2 ** 31, "table: NL * T * F must be below 2^31")
    try:
        hash_grid_resolutions(NL, base_resolution, growth)
    except ValueError as e:
        raise RuntimeError(str(e)) from None
    return (int(base_resolution), log2T, NL, F, _hash_grid_q(growth), TEX_FILTERS[filter_mode], TEX_BOUNDARIES[boundary_mode]), NL * F


# The chain checks of the two mip-mapped ops: (the table's words, B, max_mip_level) -> (the ABI words, mip's shape).
def _texture_chain(words, B, max_mip_level):
    Ht, Wt, C, per_view, _, boundary = words
    _, _, T = mip_layout(Ht, Wt, max_mip_level)
    _bad(Ht * Wt + T >= 2 ** 31, "tex: the texels of all levels must number below 2^31")
    return (Ht, Wt, C, per_view, boundary, _max_level_code(max_mip_level)), ((B,) if per_view else ()) + (T, C)


def _cube_chain(words, B, max_mip_level):
    N, C, per_view, _ = words
    _, _, T = mip_layout(N, N, max_mip_level)
    _bad(6 * (N * N + T) >= 2 ** 31, "tex: the texels of all levels of the cube must number below 2^31")
    return (N, C, per_view, _max_level_code(max_mip_level)), ((B,) if per_view else ()) + (6, T, C)


class _Lookup(NamedTuple):
    """What tells one lookup op from another."""
    name: str                       # the wrappers are <name>_cuda and <name>_backward_cuda
    coord: str                      # the coordinate's name in messages, and its width k
    width: int
    table: str                      # the table's name in messages
    boundaries: Optional[dict]      # what boundary_mode may be (None: the op has none)
    check_table: Callable           # one of the _*_table above
    forward: str                    # the two exports
    backward: str
    slot_input: Optional[tuple] = None      # mip-mapped ops: (name, trailing shape) of the second per-slot input ...
    check_chain: Optional[Callable] = None  # ... and one of the _*_chain above
    row: Optional[int] = None               # floats per slot of the raw coordinate gradient (None: width) and how it is cut
    split: tuple = (slice(None),)           # into what the backward returns, one index of the last axis each


_TEXTURE = _Lookup("texture", "uv", 2, "tex", TEX_BOUNDARIES, _texture_table, "dm2_texture", "dm2_texture_backward")
_TEXTURE_CUBE = _Lookup("texture_cube", "dirs", 3, "tex", None, _cube_table, "dm2_texture_cube", "dm2_texture_cube_backward")
_TEXTURE_VOLUME = _Lookup("texture_volume", "xyz", 3, "grid", TEX_BOUNDARIES, _volume_table, "dm2_texture_volume",
                          "dm2_texture_volume_backward")
_HASH_GRID = _Lookup("hash_grid", "xyz", 3, "table", TEX_BOUNDARIES, _hash_grid_table, "dm2_hash_grid", "dm2_hash_grid_backward")
_TEXTURE_MIP = _TEXTURE._replace(name="texture_mip", forward="dm2_texture_mip", backward="dm2_texture_mip_backward",
                                 slot_input=("uv_da", (4,)), check_chain=_texture_chain)
_TEXTURE_CUBE_MIP = _Lookup("texture_cube_mip", "dirs", 3, "tex", None, _cube_table, "dm2_texture_cube_mip",
                            "dm2_texture_cube_mip_backward", slot_input=("mip_level", ()), check_chain=_cube_chain, row=4,
                            split=(slice(0, 3), 3))


def _lookup_args(op, coord, table, render_layers, modes, grad_out=None, chain=None):
    """Checks of a lookup call.  modes = (filter_mode, boundary_mode, ...whatever else ``op.check_table`` takes); chain = (the
    second per-slot input, mip, max_mip_level) of a mip-mapped op -> (the ABI words (B, H, W, L, ...), C, the contiguous inputs
    in the library's order: (render_layers, coord[, slot input], table[, mip][, grad_out]), device).  Training calls this
    several times a step: a message is put together only where its check fails."""
    if modes[0] not in TEX_FILTERS:
        raise RuntimeError(f"filter_mode must be one of {sorted(TEX_FILTERS)}, got {modes[0]!r}")
    if op.boundaries is not None and modes[1] not in op.boundaries:
        raise RuntimeError(f"boundary_mode must be one of {sorted(op.boundaries)}, got {modes[1]!r}")
    if coord.dim() != 5 or coord.size(4) != op.width:
        raise RuntimeError(f"{op.coord} must have dimensions (B, H, W, L, {op.width}), got {tuple(coord.shape)}")
    B, H, W, L = coord.shape[:4]
    words, C = op.check_table(table, B, *modes)
    if render_layers is not None and tuple(render_layers.shape) != (B, H, W, L):
        raise RuntimeError(f"render_layers must have dimensions {(B, H, W, L)}, got {tuple(render_layers.shape)}")
    if grad_out is not None and tuple(grad_out.shape) != (B, H, W, L, C):
        raise RuntimeError(f"grad_out must have dimensions {(B, H, W, L, C)}, got {tuple(grad_out.shape)}")
    dev = _require_gpu(*[t for t in (coord, table, render_layers, grad_out) if t is not None])
    f32, i32 = torch.float32, torch.int32
    for name, t, dt in ((op.coord, coord, f32), (op.table, table, f32), ("render_layers", render_layers, i32), ("grad_out", grad_out, f32)):
        if t is not None and t.dtype != dt:
            raise RuntimeError(f"{name}: expected dtype {dt}, got {t.dtype}")
    ins = (None if render_layers is None else render_layers.contiguous(), coord.contiguous(), table.contiguous())
    if chain is not None:
        (name, tail), (slot, mip, max_mip_level) = op.slot_input, chain
        if tuple(slot.shape) != (B, H, W, L) + tail:
            raise RuntimeError(f"{name} must have dimensions {(B, H, W, L) + tail}, got {tuple(slot.shape)}")
        words, shape = op.check_chain(words, B, max_mip_level)
        if tuple(mip.shape) != shape:
            raise RuntimeError(f"mip must have dimensions {shape} for tex {tuple(table.shape)} and max_mip_level {max_mip_level}, "
                               f"got {tuple(mip.shape)}")
        _require_gpu(coord, slot, mip)
        for name, t in ((name, slot), ("mip", mip)):
            if t.dtype != f32:
                raise RuntimeError(f"{name}: expected dtype {f32}, got {t.dtype}")
        ins = (ins[0], ins[1], slot.contiguous(), ins[2], mip.contiguous())
    if grad_out is not None:
        ins += (grad_out.contiguous(),)
    return (B, H, W, L) + words, C, ins, dev


def _lookup_forward(op, coord, table, render_layers, modes, chain=None):
    lib = load_library()
    sizes, C, ins, dev = _lookup_args(op, coord, table, render_layers, modes, None, chain)
    B, H, W, L = sizes[:4]
    if B * H * W * L == 0:
        return torch.zeros((B, H, W, L, C), dtype=torch.float32, device=dev)      # no launch
    out = torch.empty((B, H, W, L, C), dtype=torch.float32, device=dev)         # (every element written by the kernel)
    with torch.cuda.device(dev):
        if getattr(lib, op.forward)(*sizes, *map(_ptr, ins), _ptr(out), _stream(dev)):
            raise _err(lib, op.name + "_cuda")
    return out


def _lookup_backward(op, coord, table, render_layers, modes, grad_out, need_tables, need_coords, chain=None):
    """need_tables: a flag per table (the table[, mip]), need_coords: a flag per entry of ``op.split`` -> their gradients in that
    order, None where not asked for."""
    lib = load_library()
    sizes, _, ins, dev = _lookup_args(op, coord, table, render_layers, modes, grad_out, chain)
    B, H, W, L = sizes[:4]
    f32 = torch.float32
    if not (any(need_tables) or any(need_coords)):
        return (None,) * (len(need_tables) + len(need_coords))
    dtables = (torch.zeros(tuple(table.shape), dtype=f32, device=dev) if need_tables[0] else None,)         # (summed into)
    if chain is not None:
        dtables += (torch.zeros(tuple(chain[1].shape), dtype=f32, device=dev) if need_tables[1] else None,)
    rows = None
    if any(need_coords):                                                  # (every element written; an empty grid launches nothing)
        rows = (torch.zeros if B * H * W * L == 0 else torch.empty)((B, H, W, L, op.row or op.width), dtype=f32, device=dev)
    if B * H * W * L != 0:
        with torch.cuda.device(dev):
            if getattr(lib, op.backward)(*sizes, *map(_ptr, ins), *map(_ptr, dtables), _ptr(rows), _stream(dev)):
                raise _err(lib, op.name + "_backward_cuda")
    if op.row is None:
        return dtables + (rows,)
    return dtables + tuple(rows[..., s].contiguous() if need else None for s, need in zip(op.split, need_coords))


def texture_cuda(uv, tex, render_layers=None, filter_mode="linear", boundary_mode="wrap"):
    """A texture sampled at per-slot UVs (include/dm2_hip.h: dm2_texture).

    uv (B,H,W,L,2) float32, tex (Ht,Wt,C) or (B,Ht,Wt,C) float32 channel-last, render_layers (B,H,W,L) int32 or None
    -> out (B,H,W,L,C) float32; 0 where the id is negative or uv is not finite (or beyond 2^24 texels)."""
    return _lookup_forward(_TEXTURE, uv, tex, render_layers, (filter_mode, boundary_mode))


def texture_backward_cuda(uv, tex, render_layers, filter_mode, boundary_mode, grad_out, need_tex, need_uv):
    """Gradients of texture_cuda (dm2_texture_backward) -> (dL_dtex of tex's shape or None, dL_duv (B,H,W,L,2) or None): only
    what ``need_tex`` / ``need_uv`` ask for is computed."""
    return _lookup_backward(_TEXTURE, uv, tex, render_layers, (filter_mode, boundary_mode), grad_out, (need_tex,), (need_uv,))


def texture_cube_cuda(dirs, tex, render_layers=None, filter_mode="linear"):
    """A cube map looked up by per-slot directions (include/dm2_hip.h: dm2_texture_cube).

    dirs (B,H,W,L,3) float32 of any non-zero length, tex (6,N,N,C) or (B,6,N,N,C) float32 channel-last (+x, -x, +y, -y, +z,
    -z), render_layers (B,H,W,L) int32 or None -> out (B,H,W,L,C) float32; 0 where the id is negative or the direction is
    not finite or all zero."""
    return _lookup_forward(_TEXTURE_CUBE, dirs, tex, render_layers, (filter_mode, None))


def texture_cube_backward_cuda(dirs, tex, render_layers, filter_mode, grad_out, need_tex, need_dirs):
    """Gradients of texture_cube_cuda (dm2_texture_cube_backward) -> (dL_dtex of tex's shape or None, dL_ddirs (B,H,W,L,3) or
    None): only what ``need_tex`` / ``need_dirs`` ask for is computed."""
    return _lookup_backward(_TEXTURE_CUBE, dirs, tex, render_layers, (filter_mode, None), grad_out, (need_tex,), (need_dirs,))


def texture_volume_cuda(xyz, grid, render_layers=None, filter_mode="linear", boundary_mode="clamp"):
    """A voxel grid looked up by per-slot positions (include/dm2_hip.h: dm2_texture_volume).

    xyz (B,H,W,L,3) float32 in the grid's unit cube (x along the grid's last spatial axis), grid (N,N,N,C) or (B,N,N,N,C)
    float32 channel-last, render_layers (B,H,W,L) int32 or None -> out (B,H,W,L,C) float32; 0 where the id is negative or a
    coordinate is not finite (or beyond 2^24 voxels)."""
    return _lookup_forward(_TEXTURE_VOLUME, xyz, grid, render_layers, (filter_mode, boundary_mode))


def texture_volume_backward_cuda(xyz, grid, render_layers, filter_mode, boundary_mode, grad_out, need_grid, need_xyz):
    """Gradients of texture_volume_cuda (dm2_texture_volume_backward) -> (dL_dgrid of grid's shape or None,
    dL_dxyz (B,H,W,L,3) or None): only what ``need_grid`` / ``need_xyz`` ask for is computed."""
    return _lookup_backward(_TEXTURE_VOLUME, xyz, grid, render_layers, (filter_mode, boundary_mode), grad_out, (need_grid,),
                            (need_xyz,))


def hash_grid_cuda(xyz, table, render_layers=None, base_resolution=16, growth=1.5, filter_mode="linear", boundary_mode="clamp"):
    """A multiresolution hash encoding looked up by per-slot positions (include/dm2_hip.h: dm2_hash_grid).

    xyz (B,H,W,L,3) float32 in the field's unit cube, table (NL,T,F) float32, render_layers (B,H,W,L) int32 or None -> out
    (B,H,W,L,NL*F) float32, channel l * F + f; 0 where the id is negative or a coordinate is not finite (or beyond 2^24 voxels
    of the finest level)."""
    return _lookup_forward(_HASH_GRID, xyz, table, render_layers, (filter_mode, boundary_mode, base_resolution, growth))


def hash_grid_backward_cuda(xyz, table, render_layers, base_resolution, growth, filter_mode, boundary_mode, grad_out, need_table,
                            need_xyz):
    """Gradients of hash_grid_cuda (dm2_hash_grid_backward) -> (dL_dtable (NL,T,F) or None,
    dL_dxyz (B,H,W,L,3) or None): only what ``need_table`` / ``need_xyz`` ask for is computed."""
    return _lookup_backward(_HASH_GRID, xyz, table, render_layers, (filter_mode, boundary_mode, base_resolution, growth), grad_out,
                            (need_table,), (need_xyz,))


def texture_mip_cuda(uv, uv_da, tex, mip, render_layers=None, boundary_mode="wrap", max_mip_level=None):
    """Trilinear sampling of a texture and its mip chain (include/dm2_hip.h: dm2_texture_mip).

    uv (B,H,W,L,2), uv_da (B,H,W,L,4) = (du/dX, dv/dX, du/dY, dv/dY), tex (Ht,Wt,C) or (B,Ht,Wt,C), mip = texture_mipmaps_cuda's
    chain of tex under the same max_mip_level, render_layers (B,H,W,L) int32 or None -> out (B,H,W,L,C) float32; 0 where the id is
    negative or uv / uv_da is not finite."""
    return _lookup_forward(_TEXTURE_MIP, uv, tex, render_layers, ("linear", boundary_mode), (uv_da, mip, max_mip_level))


def texture_mip_backward_cuda(uv, uv_da, tex, mip, render_layers, boundary_mode, max_mip_level, grad_out, need_tex, need_mip, need_uv):
    """Gradients of texture_mip_cuda (dm2_texture_mip_backward) -> (dL_dtex of tex's shape, dL_dmip of mip's shape, dL_duv
    (B,H,W,L,2)), each None unless its ``need_*`` asks for it; uv_da gets none (the level of detail is a constant of the op)."""
    return _lookup_backward(_TEXTURE_MIP, uv, tex, render_layers, ("linear", boundary_mode), grad_out, (need_tex, need_mip),
                            (need_uv,), (uv_da, mip, max_mip_level))


def texture_cube_mip_cuda(dirs, level, tex, mip, render_layers=None, max_mip_level=None):
    """A cube map and its mip chain looked up by per-slot directions and levels of detail (include/dm2_hip.h:
    dm2_texture_cube_mip).

    dirs (B,H,W,L,3), level (B,H,W,L) float32 (level 0 is tex), tex (6,N,N,C) or (B,6,N,N,C), mip (6,T,C) or (B,6,T,C): per face
    the levels 1 .. nlev-1 in ``mip_layout(N, N, max_mip_level)``'s packing, render_layers (B,H,W,L) int32 or None -> out
    (B,H,W,L,C) float32; 0 where the id is negative, the direction is not finite or all zero, or the level is not finite."""
    return _lookup_forward(_TEXTURE_CUBE_MIP, dirs, tex, render_layers, ("linear", None), (level, mip, max_mip_level))


def texture_cube_mip_backward_cuda(dirs, level, tex, mip, render_layers, max_mip_level, grad_out, need_tex, need_mip, need_dirs,
                                   need_level):
    """Gradients of texture_cube_mip_cuda (dm2_texture_cube_mip_backward) -> (dL_dtex of tex's shape,
    dL_dmip of mip's shape, dL_ddirs (B,H,W,L,3), dL_dlevel (B,H,W,L)), each None unless its ``need_*`` asks for it.  The
    direction's and the level's gradients come from one kernel as rows of four floats, split here."""
    return _lookup_backward(_TEXTURE_CUBE_MIP, dirs, tex, render_layers, ("linear", None), grad_out, (need_tex, need_mip),
                            (need_dirs, need_level), (level, mip, max_mip_level))


def _vertex_normals_args(verts, faces, offsets, corners, normals=None, lens=None, grad_normals=None):
    """Checks of a vertex-normals call -> ((P, F), contiguous tensors, device)."""
    _bad(verts.dim() != 2 or verts.size(1) != 3, f"verts must have dimensions (P, 3), got {tuple(verts.shape)}")
    _bad(faces.dim() != 2 or faces.size(1) != 3, f"faces must have dimensions (F, 3), got {tuple(faces.shape)}")
    P, F = int(verts.size(0)), int(faces.size(0))
    _bad(3 * F >= 2 ** 31, "faces: 3 * F must be below 2^31")
    _bad(tuple(offsets.shape) != (P + 1,), f"offsets must have dimensions ({P + 1},), got {tuple(offsets.shape)}")
    _bad(tuple(corners.shape) != (3 * F,), f"corners must have dimensions ({3 * F},), got {tuple(corners.shape)}")
    for name, t, shape in (("normals", normals, (P, 3)), ("len", lens, (P,)), ("grad_normals", grad_normals, (P, 3))):
        _bad(t is not None and tuple(t.shape) != shape, f"{name} must have dimensions {shape}, got {tuple(t.shape) if t is not None else None}")
    f32, i32 = torch.float32, torch.int32
    named = (("verts", verts, f32), ("faces", faces, i32), ("offsets", offsets, i32), ("corners", corners, i32),
             ("normals", normals, f32), ("len", lens, f32), ("grad_normals", grad_normals, f32))
    dev = _require_gpu(*[t for _, t, _ in named if t is not None])
    ts = []
    for name, t, dt in named:
        _bad(t is not None and t.dtype != dt, f"{name}: expected dtype {dt}, got {t.dtype if t is not None else None}")
        ts.append(None if t is None else t.contiguous())
    return (P, F), ts, dev


def vertex_normals_cuda(verts, faces, offsets, corners, normalize=True):
    """Area-weighted vertex normals without atomics (include/dm2_hip.h: dm2_vertex_normals).

    verts (P,3) float32, faces (F,3) int32, (offsets (P+1,), corners (3F,)) int32 = ``Renderer.vertex_adjacency(faces, P)`` ->
    (normals (P,3) float32, len (P,) float32 = the length of each vertex's summed face normals, what the backward takes)."""
    lib = load_library()
    (P, F), (vc, fc, of, co, _, _, _), dev = _vertex_normals_args(verts, faces, offsets, corners)
    f32 = torch.float32
    normals = torch.empty((P, 3), dtype=f32, device=dev)                      # (every element written by the kernel)
    lens = torch.empty((P,), dtype=f32, device=dev)
    if P == 0:
        return normals, lens
    nbytes = lib.dm2_vertex_normals_scratch_bytes(P, F, 0)
    scratch = _bytes(dev, nbytes)
    with torch.cuda.device(dev):
        if lib.dm2_vertex_normals(P, F, 1 if normalize else 0, _ptr(vc), _ptr(fc), _ptr(of), _ptr(co), _ptr(scratch), nbytes,
                                  _ptr(normals), _ptr(lens), _stream(dev)):
            raise _err(lib, "vertex_normals_cuda")
    return normals, lens


def vertex_normals_backward_cuda(verts, faces, offsets, corners, normalize, normals, lens, grad_normals):
    """Gradient of vertex_normals_cuda (dm2_vertex_normals_backward) for grad_normals (P,3) -> dL_dverts (P,3); ``normals`` and
    ``lens`` are the forward's (``lens`` decides which vertices are zero; the normal itself is evaluated again in double from
    ``verts``).  No atomics: the same bits on every call."""
    lib = load_library()
    (P, F), (vc, fc, of, co, nr, ln, gn), dev = _vertex_normals_args(verts, faces, offsets, corners, normals, lens, grad_normals)
    dverts = torch.empty((P, 3), dtype=torch.float32, device=dev)               # (every element written by the kernel)
    if P == 0:
        return dverts
    nbytes = lib.dm2_vertex_normals_scratch_bytes(P, F, 1)
    scratch = _bytes(dev, nbytes)
    with torch.cuda.device(dev):
        if lib.dm2_vertex_normals_backward(P, F, 1 if normalize else 0, _ptr(vc), _ptr(fc), _ptr(of), _ptr(co), _ptr(nr), _ptr(ln),
                                           _ptr(gn), _ptr(scratch), nbytes, _ptr(dverts), _stream(dev)):
            raise _err(lib, "vertex_normals_backward_cuda")
    return dverts


def _shading_args(render_layers, t, normals, image_ray_o, image_ray_d, grads=()):
    """Checks of a shading-vectors call -> ((B, H, W, L, flags), contiguous tensors, device, keep-alive list, window)."""
    _bad(render_layers.dim() != 4, f"render_layers must have dimensions (B, H, W, L), got {tuple(render_layers.shape)}")
    B, H, W, L = (int(x) for x in render_layers.shape)
    _bad(tuple(t.shape) != (B, H, W, L), f"t must have dimensions {(B, H, W, L)}, got {tuple(t.shape)}")
    _bad(normals is not None and tuple(normals.shape) != (B, H, W, L, 3),
        f"normals must have dimensions {(B, H, W, L, 3)}, got {tuple(normals.shape) if normals is not None else None}")
    for name, g in grads:
        _bad(g is not None and tuple(g.shape) != (B, H, W, L, 3),
            f"{name} must have dimensions {(B, H, W, L, 3)}, got {tuple(g.shape) if g is not None else None}")
    f32, i32 = torch.float32, torch.int32
    named = (("render_layers", render_layers, i32), ("t", t, f32), ("normals", normals, f32), ("image_ray_o", image_ray_o, f32),
             ("image_ray_d", image_ray_d, f32)) + tuple((name, g, f32) for name, g in grads)
    dev = _require_gpu(*[x for _, x, _ in named if x is not None])
    ana = _analytic(B, dev)
    _bad(ana is None and (tuple(image_ray_o.shape) != (B, H, W, 3) or tuple(image_ray_d.shape) != (B, H, W, 3)),
        f"image_ray_o/image_ray_d must have dimensions {(B, H, W, 3)}")
    ts = []
    for name, x, dt in named:
        _bad(x is not None and x.dtype != dt, f"{name}: expected dtype {dt}, got {x.dtype if x is not None else None}")
        ts.append(None if x is None else x.contiguous())
    keep: list = []
    flags = 0
    if ana is not None:
        if (ana[1], ana[2]) != _frame_size(W, H):
            raise RuntimeError("analytic_rays: the image size differs from render_layers' width / height")
        flags = DM2_FLAG_ANALYTIC_RAYS
        ts[3] = ts[4] = None
    ts.append(None if ana is None else ana[0])
    win = _window(B, W, H, dev, keep)
    return (B, H, W, L, flags), ts, dev, keep, win


def shading_vectors_cuda(render_layers, t, normals, image_ray_o, image_ray_d):
    """Per-slot shading vectors (include/dm2_hip.h: dm2_shading_vectors_window).

    render_layers (B,H,W,L) int32, t (B,H,W,L) float32, normals (B,H,W,L,3) float32 or None, image_ray_o / image_ray_d
    (B,H,W,3) float32 (placeholders under ``analytic_rays``; under ``window`` the window's cut) -> (position, view) or
    (position, view, normal, reflection), each (B,H,W,L,3) float32; zeros in an empty slot (a negative id or a t that is not
    finite)."""
    lib = load_library()
    sizes, (rl, tt, nr, ro, rd, cam), dev, keep, win = _shading_args(render_layers, t, normals, image_ray_o, image_ray_d)
    B, H, W, L = sizes[:4]
    n_out = 2 if nr is None else 4
    outs = tuple(torch.empty((B, H, W, L, 3), dtype=torch.float32, device=dev) for _ in range(n_out))   # (every element written)
    if B * H * W * L == 0:
        return outs
    with torch.cuda.device(dev):
        if lib.dm2_shading_vectors_window(*sizes, _win(win), _ptr(rl), _ptr(tt), _ptr(nr), _ptr(ro),
                                          _ptr(rd), _ptr(cam), *(_ptr(o) for o in outs), *((None, None) if nr is None else ()),
                                          _stream(dev)):
            raise _err(lib, "shading_vectors_cuda")
    return outs


def shading_vectors_backward_cuda(render_layers, t, normals, image_ray_o, image_ray_d, g_position, g_normal, g_reflection, need_t,
                                  need_normals):
    """Gradients of shading_vectors_cuda (dm2_shading_vectors_backward_window): upstream gradients (B,H,W,L,3) or None ->
    (dL_dt (B,H,W,L) or None, dL_dnormals (B,H,W,L,3) or None): only what ``need_t`` / ``need_normals`` ask for, and only where
    an upstream gradient reaches it (t: g_position; normals: g_normal or g_reflection), is computed; otherwise None."""
    lib = load_library()
    grads = (("g_position", g_position), ("g_normal", g_normal), ("g_reflection", g_reflection))
    sizes, (rl, tt, nr, ro, rd, gp, gn, gr, cam), dev, keep, win = _shading_args(render_layers, t, normals, image_ray_o, image_ray_d,
                                                                                  grads)
    B, H, W, L = sizes[:4]
    need_t = bool(need_t) and gp is not None
    need_normals = bool(need_normals) and nr is not None and (gn is not None or gr is not None)
    if not (need_t or need_normals):
        return None, None
    f32 = torch.float32
    dt = torch.empty((B, H, W, L), dtype=f32, device=dev) if need_t else None                 # (every element written)
    dn = torch.empty((B, H, W, L, 3), dtype=f32, device=dev) if need_normals else None
    if B * H * W * L == 0:
        return dt, dn
    with torch.cuda.device(dev):
        if lib.dm2_shading_vectors_backward_window(*sizes, _win(win), _ptr(rl), _ptr(tt), _ptr(nr),
                                                   _ptr(ro), _ptr(rd), _ptr(cam), _ptr(gp), _ptr(gn), _ptr(gr), _ptr(dt), _ptr(dn),
                                                   _stream(dev)):
            raise _err(lib, "shading_vectors_backward_cuda")
    return dt, dn


def bary_derivatives_cuda(render_layers, verts, faces, ray_cam):
    """The footprint of a pixel on each listed face (include/dm2_hip.h: dm2_bary_derivatives_window).

    render_layers (B,H,W,L) int32, verts (P,3) float32, faces (F,3) int32, ray_cam (B,32) float32 = inv(mv) then inv(proj) of
    each view -> (dbary_dx, dbary_dy), each (B,H,W,L,3) float32: the derivatives of (1 - u - v, u, v) with respect to the
    pixel's x and y.  Under ``_C.window`` render_layers is a window's and the frame is the window's; otherwise the frame is
    (W, H).  Zeros in an empty slot (id outside [0, F) or a vertex outside [0, P)) and where the ray lies in the face's plane."""
    lib = load_library()
    _bad(render_layers.dim() != 4, f"render_layers must have dimensions (B, H, W, L), got {tuple(render_layers.shape)}")
    B, H, W, L = (int(x) for x in render_layers.shape)
    _bad(verts.dim() != 2 or verts.size(1) != 3, f"verts must have dimensions (P, 3), got {tuple(verts.shape)}")
    _bad(faces.dim() != 2 or faces.size(1) != 3, f"faces must have dimensions (F, 3), got {tuple(faces.shape)}")
    _bad(tuple(ray_cam.shape) != (B, 32), f"ray_cam must have dimensions ({B}, 32), got {tuple(ray_cam.shape)}")
    f32, i32 = torch.float32, torch.int32
    named = (("render_layers", render_layers, i32), ("verts", verts, f32), ("faces", faces, i32), ("ray_cam", ray_cam, f32))
    dev = _require_gpu(*[t for _, t, _ in named])
    ts = []
    for name, t, dt in named:
        _bad(t.dtype != dt, f"{name}: expected dtype {dt}, got {t.dtype}")
        ts.append(t.contiguous())
    rl, vs, fc, cam = ts
    dx = torch.empty((B, H, W, L, 3), dtype=f32, device=dev)               # (every element written by the kernel)
    dy = torch.empty((B, H, W, L, 3), dtype=f32, device=dev)
    if B * H * W * L == 0:
        return dx, dy                                                      # no launch
    keep: list = []
    win = _window(B, W, H, dev, keep)
    with torch.cuda.device(dev):
        if lib.dm2_bary_derivatives_window(B, H, W, L, int(verts.size(0)), int(faces.size(0)), _win(win),
                                           _ptr(rl), _ptr(vs), _ptr(fc), _ptr(cam), _ptr(dx), _ptr(dy), _stream(dev)):
            raise _err(lib, "bary_derivatives_cuda")
    return dx, dy


def mip_layout(Ht, Wt, max_mip_level=None):
    """The mip chain of an (Ht, Wt) texture (include/dm2_hip.h: dm2_texture_mipmaps) -> (nlev, [(H_k, W_k, offset_k) for k = 0 ..
    nlev-1], T): level k+1 exists while both extents of level k are even and k < max_mip_level; offset_k = the first texel of
    level k >= 1 in the packed chain (level 0 is the texture itself: offset 0 by convention), T = the chain's texels."""
    if max_mip_level is not None and int(max_mip_level) < 0:
        raise ValueError("max_mip_level must not be negative")
    h, w, off, levels = int(Ht), int(Wt), 0, [(int(Ht), int(Wt), 0)]
    while h >= 1 and w >= 1 and h % 2 == 0 and w % 2 == 0 and (max_mip_level is None or len(levels) - 1 < int(max_mip_level)):
        h, w = h // 2, w // 2
        levels.append((h, w, off))
        off += h * w
    return len(levels), levels, off


def _max_level_code(max_mip_level):
    return -1 if max_mip_level is None else min(int(max_mip_level), 64)


def _mipmap_args(tex, max_mip_level, grad_mip=None):
    """Checks of a mip chain call -> (sizes (NB, Ht, Wt, C, max level code), T, contiguous tensors, device)."""
    _bad(tex.dim() not in (3, 4), "tex must have dimensions (Ht, Wt, C) or (B, Ht, Wt, C)")
    Ht, Wt, C = (int(x) for x in tex.shape[-3:])
    _bad(Ht < 1 or Wt < 1, "tex must have at least one row and one column")
    _bad(C < 1, "tex must have at least one channel")
    _, _, T = mip_layout(Ht, Wt, max_mip_level)
    _bad(Ht * Wt + T >= 2 ** 31, "tex: the texels of all levels must number below 2^31")
    NB = int(tex.size(0)) if tex.dim() == 4 else 1
    shape = ((NB,) if tex.dim() == 4 else ()) + (T, C)
    _bad(grad_mip is not None and tuple(grad_mip.shape) != shape,
        f"grad_mip must have dimensions {shape}, got {tuple(grad_mip.shape) if grad_mip is not None else None}")
    dev = _require_gpu(*[t for t in (tex, grad_mip) if t is not None])
    ts = []
    for name, t in (("tex", tex), ("grad_mip", grad_mip)):
        _bad(t is not None and t.dtype != torch.float32, f"{name}: expected dtype {torch.float32}, got {t.dtype if t is not None else None}")
        ts.append(None if t is None else t.contiguous())
    return (NB, Ht, Wt, C, _max_level_code(max_mip_level)), shape, ts, dev


def _chain_run(lib, export, what, sizes, src, shape, dev):
    """dst of ``shape`` = one of the two chain exports of src; an empty dst launches nothing."""
    dst = torch.empty(shape, dtype=torch.float32, device=dev)               # (every element written by the kernels)
    if dst.numel() != 0:
        with torch.cuda.device(dev):
            if getattr(lib, export)(*sizes, _ptr(src), _ptr(dst), _stream(dev)):
                raise _err(lib, what)
    return dst


def texture_mipmaps_cuda(tex, max_mip_level=None):
    """The mip chain of a texture (include/dm2_hip.h: dm2_texture_mipmaps): tex (Ht,Wt,C) or (B,Ht,Wt,C) float32 -> mip (T,C)
    or (B,T,C) float32, levels 1 .. nlev-1 concatenated (``mip_layout``); T = 0 (and no launch) when no level can be built."""
    lib = load_library()
    sizes, shape, (tx, _), dev = _mipmap_args(tex, max_mip_level)
    return _chain_run(lib, "dm2_texture_mipmaps", "texture_mipmaps_cuda", sizes, tx, shape, dev)


def texture_mipmaps_backward_cuda(tex, max_mip_level, grad_mip):
    """Gradient of texture_mipmaps_cuda (dm2_texture_mipmaps_backward) for grad_mip of mip's shape -> dL_dtex of tex's shape
    (only tex's shape is looked at).  A gather: deterministic."""
    lib = load_library()
    sizes, shape, (tx, gm), dev = _mipmap_args(tex, max_mip_level, grad_mip)
    if gm.numel() == 0:
        return torch.zeros(tuple(tex.shape), dtype=torch.float32, device=dev)
    return _chain_run(lib, "dm2_texture_mipmaps_backward", "texture_mipmaps_backward_cuda", sizes, gm, tuple(tex.shape), dev)


def _cube_prefilter_args(chain, N, max_mip_level, what="chain"):
    """Checks of a cube prefilter call -> (sizes (cubes, N, C, max level code), contiguous chain, device)."""
    N = int(N)
    _bad(N < 1, "N must be at least 1")
    _bad(chain.dim() not in (3, 4), f"{what} must have dimensions (6, T, C) or (B, 6, T, C)")
    _bad(int(chain.shape[-3]) != 6, f"{what}: a cube has six faces, got {int(chain.shape[-3])}")
    _, _, T = mip_layout(N, N, max_mip_level)
    _bad(6 * (N * N + T) >= 2 ** 31, "the texels of all levels of the cube must number below 2^31")
    C = int(chain.shape[-1])
    shape = tuple(chain.shape[:-3]) + (6, T, C)
    _bad(tuple(chain.shape) != shape,
        f"{what} must have dimensions {shape} for N {N} and max_mip_level {max_mip_level}, got {tuple(chain.shape)}")
    _bad(C < 1, f"{what} must have at least one channel")
    dev = _require_gpu(chain)
    _bad(chain.dtype != torch.float32, f"{what}: expected dtype {torch.float32}, got {chain.dtype}")
    cubes = int(chain.size(0)) if chain.dim() == 4 else 1
    _bad(cubes > 10922, f"{what}: at most 10922 cubes in one call")
    return (cubes, N, C, _max_level_code(max_mip_level)), chain.contiguous(), dev


def cube_prefilter_cuda(chain, N, max_mip_level=None):
    """The GGX prefilter of a cube's mip chain, un-normalised (include/dm2_hip.h: dm2_cube_prefilter): chain (6,T,C) or
    (B,6,T,C) float32, per face the levels 1 .. nlev-1 in ``mip_layout(N, N, max_mip_level)``'s packing -> the same shape: level k filtered from level k with the lobe of roughness k / (nlev - 1),
    y[o] = sum_s K(o,s) Om_s x[s].  A gather: deterministic; T = 0 launches nothing."""
    lib = load_library()
    sizes, x, dev = _cube_prefilter_args(chain, N, max_mip_level)
    return _chain_run(lib, "dm2_cube_prefilter", "cube_prefilter_cuda", sizes, x, tuple(x.shape), dev)


def cube_prefilter_transpose_cuda(grad, N, max_mip_level=None):
    """The transpose of cube_prefilter_cuda (dm2_cube_prefilter_backward): grad of the chain's
    shape -> xbar[s] = Om_s sum_o K(o,s) grad[o], the same shape.  A gather as well: deterministic."""
    lib = load_library()
    sizes, g, dev = _cube_prefilter_args(grad, N, max_mip_level, "grad")
    return _chain_run(lib, "dm2_cube_prefilter_backward", "cube_prefilter_transpose_cuda", sizes, g, tuple(g.shape), dev)


COMPOSITE_ALPHA_PER_SLOT, COMPOSITE_ALPHA_PER_FACE = 0, 1    # include/dm2_hip.h DM2_COMPOSITE_ALPHA_*


def _composite_args(values, alpha, render_layers, background, n_contrib=None, grad_out=None, grad_acc=None):
    """Checks of a composite call -> (sizes (B, H, W, L, C, F, alpha_mode), contiguous tensors, device)."""
    _bad(values.dim() != 5, f"values must have dimensions (B, H, W, L, C), got {tuple(values.shape)}")
    B, H, W, L, C = (int(x) for x in values.shape)
    _bad(C < 1, "values must have at least one channel")
    _bad(alpha.dim() not in (1, 4), f"alpha must have dimensions {(B, H, W, L)} (per slot) or (F,) (per face), got {tuple(alpha.shape)}")
    per_face = alpha.dim() == 1
    _bad(not per_face and tuple(alpha.shape) != (B, H, W, L),
        f"alpha must have dimensions {(B, H, W, L)} (per slot) or (F,) (per face), got {tuple(alpha.shape)}")
    _bad(per_face and render_layers is None, "a per-face alpha (F,) needs render_layers")
    _bad(render_layers is not None and tuple(render_layers.shape) != (B, H, W, L),
        f"render_layers must have dimensions {(B, H, W, L)}, got {tuple(render_layers.shape) if render_layers is not None else None}")
    _bad(background is not None and tuple(background.shape) != (C,),
        f"background must have dimensions {(C,)}, got {tuple(background.shape) if background is not None else None}")
    _bad(n_contrib is not None and tuple(n_contrib.shape) != (B, H, W),
        f"n_contrib must have dimensions {(B, H, W)}, got {tuple(n_contrib.shape) if n_contrib is not None else None}")
    _bad(grad_out is not None and tuple(grad_out.shape) != (B, H, W, C),
        f"grad_out must have dimensions {(B, H, W, C)}, got {tuple(grad_out.shape) if grad_out is not None else None}")
    _bad(grad_acc is not None and tuple(grad_acc.shape) != (B, H, W),
        f"grad_acc must have dimensions {(B, H, W)}, got {tuple(grad_acc.shape) if grad_acc is not None else None}")
    f32, i32 = torch.float32, torch.int32
    named = (("values", values, f32), ("alpha", alpha, f32), ("render_layers", render_layers, i32), ("background", background, f32),
             ("n_contrib", n_contrib, i32), ("grad_out", grad_out, f32), ("grad_acc", grad_acc, f32))
    dev = _require_gpu(*[t for _, t, _ in named if t is not None])
    ts = []
    for name, t, dt in named:
        _bad(t is not None and t.dtype != dt, f"{name}: expected dtype {dt}, got {t.dtype if t is not None else None}")
        ts.append(None if t is None else t.contiguous())
    F = int(alpha.size(0)) if per_face else 0
    return (B, H, W, L, C, F, COMPOSITE_ALPHA_PER_FACE if per_face else COMPOSITE_ALPHA_PER_SLOT), ts, dev


def composite_cuda(values, alpha, render_layers=None, background=None):
    """Per-slot values blended front to back into an image (include/dm2_hip.h: dm2_composite).

    values (B,H,W,L,C) float32, alpha (B,H,W,L) float32 per slot or (F,) float32 per face (gathered by render_layers),
    render_layers (B,H,W,L) int32 or None (per-slot alpha only), background (C,) float32 or None -> (out (B,H,W,C), acc (B,H,W)
    = 1 - T, final_T (B,H,W), n_contrib (B,H,W) int32)."""
    lib = load_library()
    sizes, (vc, al, rl, bg, _, _, _), dev = _composite_args(values, alpha, render_layers, background)
    B, H, W, L, C = sizes[:5]
    f32 = torch.float32
    if B * H * W == 0 or L == 0:                                           # nothing blends (T = 1): no launch
        out = torch.zeros((B, H, W, C), dtype=f32, device=dev) if bg is None else bg.expand(B, H, W, C).contiguous()
        return (out, torch.zeros((B, H, W), dtype=f32, device=dev), torch.ones((B, H, W), dtype=f32, device=dev),
                torch.zeros((B, H, W), dtype=torch.int32, device=dev))
    out = torch.empty((B, H, W, C), dtype=f32, device=dev)                 # (every element written by the kernel)
    acc = torch.empty((B, H, W), dtype=f32, device=dev)
    final_T = torch.empty((B, H, W), dtype=f32, device=dev)
    n_contrib = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if lib.dm2_composite(*sizes, _ptr(vc), _ptr(al), _ptr(rl), _ptr(bg), _ptr(out), _ptr(acc), _ptr(final_T), _ptr(n_contrib),
                             _stream(dev)):
            raise _err(lib, "composite_cuda")
    return out, acc, final_T, n_contrib


def composite_backward_cuda(values, alpha, render_layers, background, n_contrib, grad_out, grad_acc, need_values, need_alpha):
    """Gradients of composite_cuda (dm2_composite_backward) for grad_out (B,H,W,C) and grad_acc (B,H,W), either may be None ->
    (dL_dvalues (B,H,W,L,C) or None, dL_dalpha of alpha's shape or None): only what ``need_values`` / ``need_alpha`` ask for is
    computed; with both upstream gradients None nothing runs and both are None."""
    lib = load_library()
    sizes, (vc, al, rl, bg, nc, go, ga), dev = _composite_args(values, alpha, render_layers, background, n_contrib, grad_out, grad_acc)
    B, H, W, L, C = sizes[:5]
    f32 = torch.float32
    if not (need_values or need_alpha) or (go is None and ga is None):
        return None, None
    per_face = sizes[6] == COMPOSITE_ALPHA_PER_FACE
    if B * H * W == 0 or L == 0:
        return (torch.zeros((B, H, W, L, C), dtype=f32, device=dev) if need_values else None,
                torch.zeros(tuple(alpha.shape), dtype=f32, device=dev) if need_alpha else None)
    dvalues = torch.empty((B, H, W, L, C), dtype=f32, device=dev) if need_values else None      # (every element written)
    dalpha = None
    if need_alpha:                                                         # (per slot: every element written; per face: summed into)
        dalpha = torch.zeros(tuple(alpha.shape), dtype=f32, device=dev) if per_face else torch.empty((B, H, W, L), dtype=f32, device=dev)
    with torch.cuda.device(dev):
        if lib.dm2_composite_backward(*sizes, _ptr(vc), _ptr(al), _ptr(rl), _ptr(bg), _ptr(nc), _ptr(go), _ptr(ga), _ptr(dvalues),
                                      _ptr(dalpha), _stream(dev)):
            raise _err(lib, "composite_backward_cuda")
    return dvalues, dalpha


def _coverage_inside(inside, render_layers):
    """The ``inside`` mask of a coverage call (bool or integer, the shape of render_layers) as contiguous uint8, 1 where set."""
    if tuple(inside.shape) != tuple(render_layers.shape):
        raise RuntimeError(f"inside must have dimensions {tuple(render_layers.shape)}, got {tuple(inside.shape)}")
    if inside.dtype.is_floating_point or inside.dtype.is_complex:
        raise RuntimeError(f"inside: expected a bool or integer dtype, got {inside.dtype}")
    _require_gpu(inside, render_layers)
    return (inside != 0).to(torch.uint8).contiguous()


def _coverage_args(render_layers, verts_image, faces, temperature, grad_cov=None):
    """Checks of a coverage call -> (sizes (B, H, W, L, P, F, temperature), contiguous tensors, device)."""
    _bad(render_layers.dim() != 4, f"render_layers must have dimensions (B, H, W, L), got {tuple(render_layers.shape)}")
    B, H, W, L = (int(x) for x in render_layers.shape)
    _bad(verts_image.dim() != 3 or verts_image.size(0) != B or verts_image.size(2) != 2,
        f"verts_image must have dimensions ({B}, P, 2), got {tuple(verts_image.shape)}")
    _bad(faces.dim() != 2 or faces.size(1) != 3, f"faces must have dimensions (F, 3), got {tuple(faces.shape)}")
    _bad(grad_cov is not None and tuple(grad_cov.shape) != (B, H, W, L),
        f"grad_cov must have dimensions {(B, H, W, L)}, got {tuple(grad_cov.shape) if grad_cov is not None else None}")
    temperature = float(temperature)
    if not (0.0 <= temperature <= 1.0):
        raise ValueError("temperature must be in the range [0, 1]")
    f32, i32 = torch.float32, torch.int32
    named = (("render_layers", render_layers, i32), ("verts_image", verts_image, f32), ("faces", faces, i32), ("grad_cov", grad_cov, f32))
    dev = _require_gpu(*[t for _, t, _ in named if t is not None])
    ts = []
    for name, t, dt in named:
        _bad(t is not None and t.dtype != dt, f"{name}: expected dtype {dt}, got {t.dtype if t is not None else None}")
        ts.append(None if t is None else t.contiguous())
    return (B, H, W, L, int(verts_image.size(1)), int(faces.size(0)), temperature), ts, dev


def coverage_cuda(render_layers, verts_image, faces, temperature=1.0, inside=None):
    """The analytic pixel coverage of every listed slot (include/dm2_hip.h: dm2_coverage).

    render_layers (B,H,W,L) int32 face ids over the full frame, verts_image (B,P,2) float32, faces (F,3) int32, temperature in
    [0, 1] (ValueError otherwise) -> cov (B,H,W,L) float32: 0 in an empty slot and where the triangle misses the pixel, else
    (1 - temperature) + area * temperature.  ``inside`` (B,H,W,L) bool or integer (``rasterize(overlap=True)``'s): a non-empty
    slot where it is 0 gets area * temperature instead (dm2_coverage's inside)."""
    lib = load_library()
    sizes, (rl, vi, fc, _), dev = _coverage_args(render_layers, verts_image, faces, temperature)
    ins = None if inside is None else _coverage_inside(inside, render_layers)
    B, H, W, L = sizes[:4]
    cov = torch.empty((B, H, W, L), dtype=torch.float32, device=dev)       # (every element written by the kernel)
    if B * H * W * L == 0:
        return cov
    keep: list = []
    win = _window(B, W, H, dev, keep)                    # (then render_layers is the window's, verts_image the frame's)
    with torch.cuda.device(dev):
        if lib.dm2_coverage(*sizes, _win(win), _ptr(rl), _ptr(ins), _ptr(vi), _ptr(fc), _ptr(cov), _stream(dev)):
            raise _err(lib, "coverage_cuda")
    return cov


def coverage_backward_cuda(render_layers, verts_image, faces, temperature, grad_cov):
    """Gradient of coverage_cuda (dm2_coverage_backward) for grad_cov (B,H,W,L) -> dL_dverts_image (B,P,2), or None where
    nothing flows: grad_cov None or temperature == 0 (no kernel runs)."""
    lib = load_library()
    sizes, (rl, vi, fc, gc), dev = _coverage_args(render_layers, verts_image, faces, temperature, grad_cov)
    if gc is None or sizes[6] == 0.0:
        return None
    B, H, W, L, P, F = sizes[:6]
    dimage = torch.zeros((B, P, 2), dtype=torch.float32, device=dev)       # (summed into)
    if B * H * W * L == 0 or P == 0 or F == 0:
        return dimage
    keep: list = []
    win = _window(B, W, H, dev, keep)
    with torch.cuda.device(dev):
        if lib.dm2_coverage_backward(*sizes, _win(win), _ptr(rl), _ptr(vi), _ptr(fc), _ptr(gc), _ptr(dimage), _stream(dev)):
            raise _err(lib, "coverage_backward_cuda")
    return dimage


def _composite_desc(render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background,
                    image_ray_o, image_ray_d, keep):
    """Checks (in the style of generate_render_layers_cuda) + the dm2_layer_composite_desc of a composite call."""
    _bad(render_layers.dim() != 4, "render_layers must have dimensions (B, H, W, L)")
    _bad(verts.dim() != 2 or verts.size(1) != 3, "verts must have dimensions (P, 3)")
    _bad(faces.dim() != 2 or faces.size(1) != 3, "faces must have dimensions (F, 3)")
    _bad(verts_color.dim() != 2 or verts_color.size(1) != 3, "vert color must have dimensions (P, 3)")
    _bad(faces_opacity.dim() != 1 or faces_opacity.size(0) != faces.size(0), "face opacity must have dimensions (F,)")
    _bad(faces_intense.dim() != 2 or faces_intense.size(1) != faces.size(0), "faces_intense must have dimensions (B, F,)")
    _bad(verts_ndc.dim() != 3 or verts_ndc.size(2) != 3, "verts_ndc must have dimensions (B, P, 3)")
    _bad(background.dim() != 1 or background.size(0) != 3, "background must have dimensions (3,)")
    _bad(image_ray_o.dim() != 4 or image_ray_o.size(3) != 3, "image_ray_o must have dimensions (B, H, W, 3)")
    _bad(image_ray_d.dim() != 4 or image_ray_d.size(3) != 3, "image_ray_d must have dimensions (B, H, W, 3)")
    dev = _require_gpu(render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background,
                       image_ray_o, image_ray_d)
    f32, i32 = torch.float32, torch.int32
    B, H, W, L = (int(x) for x in render_layers.shape)
    P, F = verts.size(0), faces.size(0)
    _bad(tuple(verts_color.shape) != (P, 3), "verts_color must have dimensions (P, 3)")
    _bad(tuple(faces_intense.shape) != (B, F), "faces_intense must have dimensions (B, F)")
    _bad(tuple(verts_ndc.shape) != (B, P, 3), "verts_ndc must have dimensions (B, P, 3)")
    ana = _analytic(B, dev)
    _bad(ana is None and (tuple(image_ray_o.shape) != (B, H, W, 3) or tuple(image_ray_d.shape) != (B, H, W, 3)),
        "image_ray_o/image_ray_d must have dimensions (B, H, W, 3)")
    ts = dict(render_layers=_c(render_layers, i32), verts=_c(verts, f32), faces=_c(faces, i32), verts_color=_c(verts_color, f32),
              faces_opacity=_c(faces_opacity, f32), faces_intense=_c(faces_intense, f32), verts_ndc=_c(verts_ndc, f32),
              background=_c(background, f32), image_ray_o=_c(image_ray_o, f32), image_ray_d=_c(image_ray_d, f32))
    keep += list(ts.values())
    d = LayerCompositeDesc()
    d.B, d.P, d.F, d.W, d.H, d.L, d.flags = B, P, F, W, H, L, 0
    for k, t in ts.items():
        setattr(d, k, t.data_ptr() if t.numel() > 0 else None)
    _analytic_onto(d, ana, W, H, keep, "analytic_rays: the image size differs from render_layers' width / height")
    return d, dev


def composite_layers_cuda(render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background,
                          image_ray_o, image_ray_d):
    """Front-to-back compositing of per-pixel face layers (include/dm2_hip.h: dm2_layers_composite).

    render_layers (B,H,W,L) int32 (ids outside [0, F) are skipped), verts (P,3), faces (F,3) int32, verts_color (P,3),
    faces_opacity (F), faces_intense (B,F), verts_ndc (B,P,3), background (3), image_ray_o / image_ray_d (B,H,W,3) of the
    full frame (placeholders under ``analytic_rays``) -> (color (B,H,W,3), depth_raw (B,H,W) NDC depth with background 1,
    final_T (B,H,W), n_contrib (B,H,W) int32: 1 + index of the last layer that blended); under ``face_weights_output`` a
    fifth: face_weights (B,F), the sum of alpha * T over each face's blends (dm2_layers_composite's out_face_weights)."""
    lib = load_library()
    keep: list = []
    d, dev = _composite_desc(render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background,
                             image_ray_o, image_ray_d, keep)
    win = _window(d.B, d.W, d.H, dev, keep)              # (then render_layers and the rays are the window's)
    B, H, W = d.B, d.H, d.W
    f32 = torch.float32
    color = torch.empty((B, H, W, 3), dtype=f32, device=dev)
    depth = torch.empty((B, H, W), dtype=f32, device=dev)
    final_T = torch.empty((B, H, W), dtype=f32, device=dev)
    n_contrib = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    weights = torch.zeros((B, d.F), dtype=f32, device=dev) if getattr(_tls, "face_weights_output", False) else None
    extra = (weights,) if weights is not None else ()
    if B * H * W == 0:
        return (color, depth, final_T, n_contrib) + extra
    with torch.cuda.device(dev):
        if lib.dm2_layers_composite(ctypes.byref(d), _win(win), _ptr(color), _ptr(depth), _ptr(final_T), _ptr(n_contrib),
                                    _ptr(weights), _stream(dev)):
            raise _err(lib, "composite_layers_cuda")
    return (color, depth, final_T, n_contrib) + extra


def composite_layers_backward_cuda(render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background,
                                   image_ray_o, image_ray_d, n_contrib, dL_dcolor, dL_ddepth, dL_dout_alpha=None):
    """Gradients of composite_layers_cuda (dm2_layers_composite_backward): dL_dcolor (B,H,W,3), dL_ddepth (B,H,W) of depth_raw,
    n_contrib from the forward -> (dL_dverts_color (P,3), dL_dfaces_opacity (F), dL_dverts_ndc (B,P,3) [z only],
    dL_dfaces_intense (B,F)).  Nothing reaches verts (through the barycentrics) or background.  dL_dout_alpha (B,H,W) or
    None: the gradient of alpha = 1 - final_T (it reaches dL_dfaces_opacity only)."""
    lib = load_library()
    keep: list = []
    d, dev = _composite_desc(render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background,
                             image_ray_o, image_ray_d, keep)
    win = _window(d.B, d.W, d.H, dev, keep)              # (then render_layers and the rays are the window's)
    B, P, F, H, W = d.B, d.P, d.F, d.H, d.W
    f32 = torch.float32
    checks = [(n_contrib, (B, H, W), "n_contrib"), (dL_dcolor, (B, H, W, 3), "dL_dcolor"), (dL_ddepth, (B, H, W), "dL_ddepth")]
    if dL_dout_alpha is not None:
        checks.append((dL_dout_alpha, (B, H, W), "dL_dout_alpha"))
    for t, shape, nm in checks:
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{nm} must have dimensions {shape}, got {tuple(t.shape)}")
        _require_gpu(render_layers, t)
    nc, gc, gd = _c(n_contrib, torch.int32), _c(dL_dcolor, f32), _c(dL_ddepth, f32)
    ga = _c(dL_dout_alpha, f32) if dL_dout_alpha is not None else None
    dcolor = torch.zeros((P, 3), dtype=f32, device=dev)
    dopacity = torch.zeros((F,), dtype=f32, device=dev)
    dndc = torch.zeros((B, P, 3), dtype=f32, device=dev)
    dintense = torch.zeros((B, F), dtype=f32, device=dev)
    if B * H * W == 0:
        return dcolor, dopacity, dndc, dintense
    with torch.cuda.device(dev):
        if lib.dm2_layers_composite_backward(ctypes.byref(d), _win(win), _ptr(gc), _ptr(gd), _ptr(ga), _ptr(nc), _ptr(dcolor),
                                             _ptr(dopacity), _ptr(dndc), _ptr(dintense), _stream(dev)):
            raise _err(lib, "composite_layers_backward_cuda")
    return dcolor, dopacity, dndc, dintense

def _prep_desc(verts, faces, mv, proj, width, height, keep):
    dev = _require_gpu(verts, faces, mv, proj)
    if verts.dim() != 2 or verts.size(1) != 3:
        raise RuntimeError("verts must have dimensions (P, 3)")
    if faces.dim() != 2 or faces.size(1) != 3:
        raise RuntimeError("faces must have dimensions (F, 3)")
    if mv.dim() != 3 or tuple(mv.shape[1:]) != (4, 4) or tuple(proj.shape) != tuple(mv.shape):
        raise RuntimeError("mv and proj must have dimensions (B, 4, 4)")
    f32, i32 = torch.float32, torch.int32
    v, fc, m, pr = _c(verts, f32), _c(faces, i32), _c(mv, f32), _c(proj, f32)
    keep += [v, fc, m, pr]
    d = PrepDesc()
    d.B, d.P, d.F, d.W, d.H = m.shape[0], v.shape[0], fc.shape[0], int(width), int(height)
    d.verts, d.faces, d.mv, d.proj = _ptr(v), _ptr(fc), _ptr(m), _ptr(pr)
    return d, dev


def prepare_faces(verts, faces, mv, proj, width, height, tables=True):
    """Fused host prep (include/dm2_hip.h: dm2_prepare_faces): -> (verts_ndc (B,P,3), verts_image (B,P,2),
    aa_face_verts, aa_face_edges, aa_face_edges_iszero (bool), aa_face_edges_recip, aa_face_edges_normal
    (all (B,F,3,2)), aa_face_edges_normal_c (B,F,3)); with tables=False only the first two."""
    lib = load_library()
    keep = []
    d, dev = _prep_desc(verts, faces, mv, proj, width, height, keep)
    B, P, F = d.B, d.P, d.F
    f32 = torch.float32
    ndc = torch.empty((B, P, 3), dtype=f32, device=dev)
    image = torch.empty((B, P, 2), dtype=f32, device=dev)
    d.verts_ndc, d.verts_image = _ptr(ndc), _ptr(image)
    outs = [ndc, image]
    if tables:
        aav, aae, aar, aan = (torch.empty((B, F, 3, 2), dtype=f32, device=dev) for _ in range(4))
        aaz = torch.empty((B, F, 3, 2), dtype=torch.bool, device=dev)
        aac = torch.empty((B, F, 3), dtype=f32, device=dev)
        d.aa_face_verts, d.aa_face_edges, d.aa_face_edges_iszero = _ptr(aav), _ptr(aae), _ptr(aaz)
        d.aa_face_edges_recip, d.aa_face_edges_normal, d.aa_face_edges_normal_c = _ptr(aar), _ptr(aan), _ptr(aac)
        outs += [aav, aae, aaz, aar, aan, aac]
    with torch.cuda.device(dev):
        if lib.dm2_prepare_faces(ctypes.byref(d), _stream(dev)):
            raise _err(lib, "dm2_prepare_faces")
    return tuple(outs)


def prepare_faces_backward(verts, faces, mv, proj, width, height, g_verts_ndc=None, g_verts_image=None, g_aa_face_verts=None,
                           need_verts=True, need_camera=False):
    """d(verts) (P,3) through the fused host prep (dm2_prepare_faces_backward).  With ``need_camera=True``: (d(verts) or None
    when ``need_verts=False``, d(mv) (B,4,4), d(proj) (B,4,4)) -- dm2_prepare_faces_backward_camera."""
    lib = load_library()
    keep = []
    d, dev = _prep_desc(verts, faces, mv, proj, width, height, keep)
    f32 = torch.float32
    gs = []
    for g, shape in ((g_verts_ndc, (d.B, d.P, 3)), (g_verts_image, (d.B, d.P, 2)), (g_aa_face_verts, (d.B, d.F, 3, 2))):
        if g is not None:
            if tuple(g.shape) != shape:
                raise RuntimeError(f"upstream gradient has shape {tuple(g.shape)}, expected {shape}")
            g = _c(g, f32)
            _require_gpu(verts, g)
        gs.append(g)
    need_verts = bool(need_verts) or not need_camera
    scratch = torch.empty((d.B * d.P * 2,), dtype=f32, device=dev) if gs[2] is not None else None
    out = torch.empty((d.P, 3), dtype=f32, device=dev) if need_verts else None
    if not need_camera:
        with torch.cuda.device(dev):
            if lib.dm2_prepare_faces_backward(ctypes.byref(d), _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(scratch), _ptr(out),
                                              _stream(dev)):
                raise _err(lib, "dm2_prepare_faces_backward")
        return out
    g_mv = torch.empty((d.B, 4, 4), dtype=f32, device=dev)
    g_proj = torch.empty((d.B, 4, 4), dtype=f32, device=dev)
    cam = _bytes(dev, lib.dm2_prepare_faces_camera_scratch_bytes(d.B, d.P))
    with torch.cuda.device(dev):
        if lib.dm2_prepare_faces_backward_camera(ctypes.byref(d), _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(scratch), _ptr(out),
                                                 _ptr(g_mv), _ptr(g_proj), _ptr(cam), _stream(dev)):
            raise _err(lib, "dm2_prepare_faces_backward_camera")
    return out, g_mv, g_proj


def debug_fetch(what, count, aux, num_rendered, scratch, dtype, n):
    """Copy an internal array out of a scratch buffer (tests only; see dm2_debug_fetch)."""
    lib = load_library()
    out = torch.empty((n,), dtype=dtype, device=scratch.device)
    if n == 0:
        return out
    with torch.cuda.device(scratch.device):
        if lib.dm2_debug_fetch(what, count, aux, num_rendered, _ptr(scratch), scratch.numel(), _ptr(out), _stream(scratch.device)):
            raise _err(lib, "debug_fetch")
    return out


def debug_aa_overlap(variant, aa_v, aa_e, aa_z, aa_r, aa_n, aa_c, pixmin):
    """Run device clipper `variant` (see dm2_debug_aa_overlap) on n (triangle, pixel) pairs; tables (n,3,2) / (n,3),
    pixmin (n,2).  -> area (n), grad (n,3,2), code (n) int32."""
    lib = load_library()
    dev = _require_gpu(aa_v, aa_e, aa_z, aa_r, aa_n, aa_c, pixmin)
    f32 = torch.float32
    n = aa_v.shape[0]
    ts = [_c(aa_v, f32), _c(aa_e, f32), _c(aa_z, torch.bool), _c(aa_r, f32), _c(aa_n, f32), _c(aa_c, f32), _c(pixmin, f32)]
    area = torch.zeros((n,), dtype=f32, device=dev)
    grad = torch.zeros((n, 3, 2), dtype=f32, device=dev)
    code = torch.zeros((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if lib.dm2_debug_aa_overlap(int(variant), n, *[_ptr(t) for t in ts], _ptr(area), _ptr(grad), _ptr(code), _stream(dev)):
            raise _err(lib, "debug_aa_overlap")
    return area, grad, code


def touched_faces(face_buf, B, F):
    """(F) bool: faces binned into at least one tile of at least one view by the forward that produced ``face_buf``
    (tiles_touched of the face scratch; dm2_debug_fetch item 8).  The sharded exchange sends only those rows."""
    t = debug_fetch(8, B * F, 1, 0, face_buf, torch.int32, B * F)
    return (t.view(B, F) != 0).any(dim=0)


# ---- device side of the sharded step's sparse exchange (include/dm2_hip.h: dm2_exchange_*) --------------------------------
def exchange_mark(face_buf, faces, B, P, N):
    """-> (flags (F + P) uint8: face flags then vertex flags, counts (N, 2) int32: rows this rank will send to every owner)."""
    lib = load_library()
    dev = _require_gpu(face_buf, faces)
    F = faces.shape[0]
    fc = _c(faces, torch.int32)
    flags = torch.empty((F + P,), dtype=torch.uint8, device=dev)
    counts = torch.empty((N, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if lib.dm2_exchange_mark(B, P, F, N, _ptr(fc), _ptr(face_buf), face_buf.numel(), _ptr(flags), _ptr(counts), _stream(dev)):
            raise _err(lib, "dm2_exchange_mark")
    return flags, counts


def exchange_pack(flags, counts, total_floats, dverts, dcolor, dopacity, dintense):
    """-> the send buffer (total_floats float32): per owner [face rows | vertex rows] (see dm2_exchange_pack)."""
    lib = load_library()
    dev = _require_gpu(flags, counts, dverts, dcolor, dopacity, dintense)
    f32 = torch.float32
    P, F, B, N = dverts.shape[0], dopacity.shape[0], dintense.shape[0], counts.shape[0]
    ts = [_c(dverts, f32), _c(dcolor, f32), _c(dopacity, f32), _c(dintense, f32)]
    send = torch.empty((int(total_floats),), dtype=f32, device=dev)
    cursors = torch.empty((N, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if lib.dm2_exchange_pack(B, P, F, N, _ptr(flags), _ptr(counts), _ptr(cursors), *[_ptr(t) for t in ts], _ptr(send), _stream(dev)):
            raise _err(lib, "dm2_exchange_pack")
    return send


def exchange_unpack(recv, recv_counts, rows, rank, B, P, F):
    """-> (slice_v (ceil(P/N), 6), slice_f (ceil(F/N), 1 + B)): the owner's sums of the received rows.  recv_counts: (N, 2)
    int32 on the HOST (a list of pairs will do)."""
    lib = load_library()
    dev = _require_gpu(recv)
    recv_counts = torch.as_tensor(recv_counts, dtype=torch.int32, device="cpu").reshape(-1, 2).contiguous()
    N = recv_counts.shape[0]
    Ps, Fs = -(-P // N), -(-F // N)
    slice_v = torch.empty((Ps, 6), dtype=torch.float32, device=dev)
    slice_f = torch.empty((Fs, 1 + B), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if lib.dm2_exchange_unpack(B, P, F, N, int(rank), _ptr(recv), ctypes.c_void_p(recv_counts.data_ptr()), int(rows), _ptr(slice_v), _ptr(slice_f),
                                   _stream(dev)):
            raise _err(lib, "dm2_exchange_unpack")
    return slice_v, slice_f
