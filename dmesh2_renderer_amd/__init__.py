"""dmesh2_renderer_amd -- MI355X-native drop-in for ``dmesh2_renderer``.

Same module surface as the reference's ``dmesh2_renderer/__init__.py``:

* ``RenderFunction``  (reference :11-177)  torch.autograd.Function, 21 inputs -> (color, depth)
* ``Renderer``        (reference :179-380) nn.Module: host prep (rays, projection, AA tables) + op
* ``LayeredRenderer`` (reference :388-451) ``generate()`` -> (render_layers, render_layers_cnt), and (not in the
  reference) ``render()``: those layers composited into (color, depth), differentiable (``LayeredCompositeFunction``)
* (not in the reference) ``Renderer.rasterize()``: the first L faces each pixel's ray hits on any triangle mesh, with
  perspective-correct barycentrics and ray distance, differentiable w.r.t. the vertices (``RasterizeFunction``), and
  ``Renderer.interpolate()``: those hits turned into an image of any C-channel vertex attribute, differentiable w.r.t.
  the attribute and the barycentrics (``InterpolateFunction``), and ``Renderer.texture()``: a channel-last texture sampled
  at such an image of UVs (bilinear or nearest, wrap or clamp), differentiable w.r.t. the texture and the UVs
  (``TextureFunction``), and ``Renderer.composite()``: such per-slot values blended front to back into an image and an
  alpha image, differentiable w.r.t. the values and the per-slot or per-face opacities (``CompositeFunction``), and
  ``Renderer.coverage()``: the analytic pixel coverage of the listed faces, the anti-aliasing factor of such a blend's
  alpha, differentiable w.r.t. the vertices and the cameras (``CoverageFunction``): what moves a silhouette; with
  ``rasterize(overlap=True)`` (``RasterizeOverlapFunction``) and ``coverage(inside=...)`` the lists also name the faces that
  only graze a pixel, and that pipeline reproduces ``Renderer.forward``'s images, silhouettes included; and mip-mapped
  filtering for ``texture`` (``filter_mode="linear-mipmap-linear"``, ``TextureMipFunction``) with the two ops that feed it:
  ``Renderer.bary_derivatives()``, the pixel's footprint on each listed face (``BaryDerivativesFunction``, a constant of
  the pipeline), and ``Renderer.texture_mipmaps()``, the chain of 2 x 2 means (``MipmapFunction``); and cube-map lookup by
  direction for ``texture`` (``boundary_mode="cube"``, ``TextureCubeFunction``): filtered across the cube's edges and corners,
  and through the cube's mip chain at a level of detail per slot (``mip_level``, ``TextureCubeMipFunction``), which receives a
  gradient: a glossy reflection whose roughness can be learned; with ``Renderer.cube_prefilter()``, the GGX prefilter that
  makes that chain a roughness chain whose last level is the diffuse irradiance (``CubePrefilterFunction``, a gather both ways);
  and what produces those directions: ``Renderer.vertex_normals()``, smooth normals that carry a gradient to the vertices
  without float atomics (``VertexNormalsFunction``, over ``Renderer.vertex_adjacency()``'s index), and
  ``Renderer.shading_vectors()``, per-slot position, view, unit normal and reflection vectors from the pixel's own ray
  (``ShadingVectorsFunction``); and ``Renderer.texture3d()``: a voxel grid of colours or features looked up at that position
  (trilinear or nearest, clamp or wrap), differentiable w.r.t. the grid and the position (``TextureVolumeFunction``): the
  appearance model that needs no UV table; and ``Renderer.hash_grid()``: the multiresolution hash encoding of that position
  (``HashGridFunction``), for fields finer than a dense grid can hold

The native work goes through ``dmesh2_renderer_amd._C`` -- a ctypes shim over
the C-ABI library ``libdm2_hip.so`` (include/dm2_hip.h) whose three functions
have the reference extension's names, argument order and tuple returns
(ext.cpp:6-9).  There is no CPU fallback: CPU tensors or a missing library
raise ``RuntimeError``.
"""
from __future__ import annotations

import contextlib
import os
from typing import List, NamedTuple, Sequence

import torch

from . import _C
from .pyrenderer import Triangles

__all__ = ["RenderFunction", "Renderer", "LayeredRenderer", "LayeredCompositeFunction", "RasterizeFunction", "InterpolateFunction",
           "TextureFunction", "CoverageFunction", "Triangles", "RasterizeOverlapFunction", "BaryDerivativesFunction",
           "MipmapFunction", "TextureMipFunction", "TextureCubeFunction", "VertexNormalsFunction", "ShadingVectorsFunction",
           "TextureCubeMipFunction", "CubePrefilterFunction", "TextureVolumeFunction", "HashGridFunction"]

# Host prep of Renderer.forward (projection + the six AA tables): the fused HIP kernels of dmesh2_renderer_amd/prep.py by
# default on GPU tensors (two kernels each way instead of ~20 torch kernels each way; verts_image differs from the torch
# GEMM's in the last bit, well inside the 1e-5 of the port's tolerance); DM2_FUSED_PREP=0 or Renderer(fused_prep=False)
# selects the reference-shaped torch ops.
_FUSED_PREP_DEFAULT = os.environ.get("DM2_FUSED_PREP", "1") != "0"
_FUSED_AA_GRAD = os.environ.get("DM2_FUSED_AA_GRAD", "1") != "0"
_TABLES_FROM_IMAGE = os.environ.get("DM2_TABLES_FROM_IMAGE", "1") != "0"     # fused prep: AA tables built inside the op's plan, never materialised
_W_EPS = 1e-4   # |w| clamp of the projection, sign kept (reference __init__.py:254-255)


class _Entered:
    """``with _Entered(a, b):`` = ``with a, b:`` for context managers put together elsewhere (entered only here)."""

    def __init__(self, *managers):
        self.managers = managers

    def __enter__(self):
        self.stack = contextlib.ExitStack()
        for m in self.managers:
            self.stack.enter_context(m)

    def __exit__(self, *exc):
        return self.stack.__exit__(*exc)


def _hold_channels(ctx, *channels, read=()):
    """In a Function's forward: keeps the thread's value of each of ``_C``'s side ``channels`` on ``ctx`` for
    ``_held_channels`` in the backward; -> the values of the channels in ``read``, which the forward looks at and the backward
    does not re-enter."""
    ctx.channels = {ch: getattr(_C._tls, ch._slot, ch._off) for ch in channels}
    return tuple(getattr(_C._tls, ch._slot, ch._off) for ch in read)


def _held_channels(ctx):
    """In the backward, ``with _held_channels(ctx):`` re-enters the channels as the forward saw them (one that was off is
    entered as off, whatever the thread holds now)."""
    entered = []
    for ch, val in ctx.channels.items():
        if ch is _C.analytic_rays:
            entered.append(ch(*(val if val is not None else (None, 0, 0))))
        elif ch is _C.window:
            entered.append(ch(*(val if val is not None else (None,))))
        else:
            entered.append(ch(val))
    return _Entered(*entered)


def _save_optional(ctx, *tensors):
    """``ctx.save_for_backward`` for tensors of which some may be None; ``_saved_optional`` gives them back, None included."""
    ctx.saved_present = [t is not None for t in tensors]
    ctx.save_for_backward(*(t for t in tensors if t is not None))


def _saved_optional(ctx):
    saved = iter(ctx.saved_tensors)
    return [next(saved) if present else None for present in ctx.saved_present]


def _image_grads(grad_color, grad_depth, shape, device):
    """Zeros for an unmaterialised colour (B,H,W,3) or depth (B,H,W) gradient, ``shape`` = (B,H,W): what the alpha-carrying
    backwards hand their kernels for an image left out of the loss."""
    if grad_color is None:
        grad_color = torch.zeros(tuple(shape) + (3,), dtype=torch.float32, device=device)
    if grad_depth is None:
        grad_depth = torch.zeros(tuple(shape), dtype=torch.float32, device=device)
    return grad_color, grad_depth


class _Window(NamedTuple):
    """A checked render window (``Renderer._window``)."""
    patch_min: torch.Tensor     # (B,2) int32 on the op's device: the (x, y) origin of each view's window in the frame
    origins: list               # the same, read back
    width: int
    height: int

    @property
    def empty(self):
        return self.width == 0 or self.height == 0


class RenderFunction(torch.autograd.Function):
    """Differentiable rasterize-and-composite op (reference __init__.py:11-177).

    Inputs (positional, as in the reference): background(3), patch_min(B,2) i32,
    patch_width, patch_height, verts(P,3)*, faces(F,3) i32, verts_color(P,3)*,
    faces_opacity(F)*, verts_ndc(B,P,3)* [grad only in z], verts_image(B,P,2),
    faces_intense(B,F)*, aa_temperature, aa_face_verts(B,F,3,2)*, aa_face_edges,
    aa_face_edges_iszero (bool), aa_face_edges_recip, aa_face_edges_normal
    (all (B,F,3,2)), aa_face_edges_normal_c(B,F,3), len_oarea_buffer,
    image_ray_o(B,H,W,3), image_ray_d(B,H,W,3).  (* = receives a gradient.)

    Outputs: (color, depth); under ``_C.alpha_output(True)`` (color, depth, alpha) with alpha (B,H,W) = 1 - T, the share
    of each pixel the blended faces cover.  Then an output left out of the loss costs nothing in the backward: an unused
    alpha launches the kernels of the two-output op.  Under ``_C.face_weights_output(True)`` one more output at the end:
    face_weights (B,F), the sum of alpha * T over each face's blends -- non-differentiable; the backward is the call it
    would be without it.
    """

    N_INPUTS = 21
    # positions (in the 21-tuple) of the inputs that get a gradient, in the
    # order render_backward_cuda returns them (render.cu:372)
    _GRAD_SLOTS = (4, 6, 7, 8, 10, 12)

    @staticmethod
    def forward(ctx, *inputs):
        if len(inputs) != RenderFunction.N_INPUTS:
            raise TypeError(f"RenderFunction takes {RenderFunction.N_INPUTS} inputs, got {len(inputs)}")
        # kept for the backward: analytic rays (Renderer(analytic_rays=True): the camera block rides along in the side channel)
        # and the fused host prep's two -- under aa_grad_to_verts the AA-corner gradients come back already scattered to the
        # vertices' image coordinates (input 9, verts_image) instead of as dL/d(aa_face_verts) (input 12)
        ctx.alpha, ctx.weights = _hold_channels(ctx, _C.analytic_rays, _C.aa_grad_to_verts, _C.tables_from_image,
                                                read=(_C.alpha_output, _C.face_weights_output))
        if ctx.alpha:
            ctx.set_materialize_grads(False)        # an unused alpha arrives as None, and the backward is the two-output one
        try:
            with _C.forward_only(not any(ctx.needs_input_grad)):
                out = _C.render_forward_cuda(*inputs)
        except Exception as ex:
            print("\nAn error occured in renderer forward.")
            print(ex)
            raise
        ctx.channels[_C.forward_mode] = _C.last_forward_mode()      # what this forward left for its backward (masks, pair pool): picks the backward's kernel
        num_rendered, color, depth = out[0], out[1], out[2]
        opaque = out[3:10]          # 4 AA-record tensors + face/binning/image byte buffers
        tensors_in = [x for x in inputs if torch.is_tensor(x)]
        ctx.save_for_backward(*tensors_in, *opaque)
        ctx.n_tensor_in = len(tensors_in)
        ctx.tensor_slots = [i for i, x in enumerate(inputs) if torch.is_tensor(x)]
        ctx.scalars = {i: x for i, x in enumerate(inputs) if not torch.is_tensor(x)}
        ctx.num_rendered = num_rendered
        res = (color, depth, out[10]) if ctx.alpha else (color, depth)
        if ctx.weights:
            ctx.mark_non_differentiable(out[-1])
            res += (out[-1],)
        return res

    @staticmethod
    def backward(ctx, grad_out_color, grad_out_depth, *grad_rest):
        # grad_rest: (alpha's,) under alpha_output, then face_weights' (non-differentiable: ignored)
        grad_out_alpha = grad_rest[0] if ctx.alpha else None
        saved = ctx.saved_tensors
        inputs: list = [None] * RenderFunction.N_INPUTS
        for slot, t in zip(ctx.tensor_slots, saved[:ctx.n_tensor_in]):
            inputs[slot] = t
        for slot, v in ctx.scalars.items():
            inputs[slot] = v
        oarea, tri_id, tri_cnt, doarea, face_buf, binning_buf, image_buf = saved[ctx.n_tensor_in:]
        if ctx.alpha:                               # (grads not materialised)
            grad_out_color, grad_out_depth = _image_grads(grad_out_color, grad_out_depth,
                                                          (int(inputs[8].shape[0]), int(inputs[3]), int(inputs[2])), inputs[8].device)
        try:
            with _held_channels(ctx):
                # (the keyword only when alpha is in the loss: otherwise the very call of the two-output op)
                extra = {} if grad_out_alpha is None else {"dL_dout_alpha": grad_out_alpha}
                grads = _C.render_backward_cuda(
                    ctx.num_rendered, *inputs, grad_out_color, grad_out_depth,
                    face_buf, binning_buf, image_buf, oarea, tri_id, tri_cnt, doarea, **extra)
        except Exception as ex:
            print("\nAn error occured in renderer backward.")
            print(ex)
            raise
        result: list = [None] * RenderFunction.N_INPUTS
        for slot, g in zip(RenderFunction._GRAD_SLOTS, grads):
            result[slot] = g
        if ctx.channels[_C.aa_grad_to_verts]:
            result[9], result[12] = grads[5], None          # (B,P,2): the gradient of verts_image, not of aa_face_verts
        return tuple(result)


class Renderer(torch.nn.Module):
    """Reference ``Renderer`` (__init__.py:179-380).

    ``mv``/``proj`` are (Bcam,4,4) column-vector matrices applied as row
    vectors (``v @ mv^T @ proj^T``).  One primary ray per pixel centre is
    precomputed for every camera at construction.

    Cameras that require grad get it, as in the reference: through the projection of ``verts`` (``verts_ndc``, the AA
    corners from ``verts_image``) on every host prep -- the fused one (dm2_prepare_faces_backward_camera) and the
    reference-shaped torch ops.  The per-pixel rays are constants: built once at construction, they get no gradient and
    are not refreshed when ``mv`` / ``proj`` change afterwards.
    """

    def __init__(self, mv, proj, width, height, device, aa_grad_buffer_size=20, fused_prep=None, analytic_rays=False,
                 tables_from_image=None):
        super().__init__()
        # not part of the reference's signature: with the fused prep, False hands the op the six materialised AA tables (the
        # reference's 21 arguments as they are); the default lets the op build them from verts_image in its plan
        self.tables_from_image = tables_from_image
        # not part of the reference's signature: analytic_rays=True keeps no (Bcam,H,W,3) ray tensors (49.8 MB per camera at
        # 1080p); the kernels compute each pixel's ray from inv(mv), inv(proj) in the operation order of _init_rays
        self.analytic_rays = bool(analytic_rays)
        self._setup(mv, proj, width, height, device)
        self.aa_grad_buffer_size = aa_grad_buffer_size
        # not part of the reference's signature: projection + AA tables by the fused HIP prep (dmesh2_renderer_amd/prep.py;
        # the default) or by the reference-shaped torch ops below (False)
        self.fused_prep = _FUSED_PREP_DEFAULT if fused_prep is None else bool(fused_prep)

    def _setup(self, mv, proj, width, height, device):
        self.mv = mv
        self.proj = proj
        self.width = width
        self.height = height
        self.device = device
        self.num_batch = mv.shape[0]
        self.ray_o = None
        self.ray_d = None
        # the rays are constants of the op, as in the reference (which returns no gradient for them): built without an autograd
        # graph, so that cameras that require grad do not tie every step's backward to a graph of the constructor
        with torch.no_grad():
            if self._analytic():
                self.ray_cam = torch.cat((torch.inverse(mv).reshape(-1, 16), torch.inverse(proj).reshape(-1, 16)), dim=1) \
                    .to(device=device, dtype=torch.float32).contiguous()
            else:
                self._init_rays()

    # -- rays ------------------------------------------------------------------
    def _init_rays(self):
        """Per-pixel world-space rays for every camera (reference :198-237).

        The ray target is the NDC point (x, y, -1, 1) taken through
        inv(proj), inv(mv) WITHOUT a perspective divide, and the direction is
        normalised with ``+1e-6`` on the length -- both as in the reference.
        """
        Bc, H, W, dev = self.num_batch, self.height, self.width, self.device
        inv_mv = torch.inverse(self.mv)
        inv_proj = torch.inverse(self.proj)
        cam_pos = inv_mv[:, :3, 3]                                           # (Bc,3)
        self.ray_o = cam_pos.reshape(Bc, 1, 1, 3).expand(Bc, H, W, 3).to(dev).contiguous()

        xs = torch.arange(W, device=dev).float() + 0.5                       # pixel centres
        ys = torch.arange(H, device=dev).float() + 0.5
        ndc_x = (xs / W * 2) - 1                                             # (W,)
        ndc_y = (ys / H * 2) - 1                                             # (H,)
        pix_h = torch.empty((Bc, H, W, 1, 4), device=dev, dtype=torch.float32)
        pix_h[..., 0, 0] = ndc_x.view(1, 1, W)
        pix_h[..., 0, 1] = ndc_y.view(1, H, 1)
        pix_h[..., 0, 2] = -1.0
        pix_h[..., 0, 3] = 1.0
        to_view = inv_proj.transpose(1, 2).unsqueeze(1).unsqueeze(1)         # (Bc,1,1,4,4)
        to_world = inv_mv.transpose(1, 2).unsqueeze(1).unsqueeze(1)
        target = torch.matmul(torch.matmul(pix_h, to_view), to_world)[..., 0, :3]   # (Bc,H,W,3), no /w
        d = target - self.ray_o
        self.ray_d = d / (torch.norm(d, dim=-1, keepdim=True) + 1e-6)

    def _camera_rows(self, t, batch_mvp_idx):
        """t[batch_mvp_idx] -- as a view (no copy) when the cameras are one or a run of consecutive ones."""
        idx = [int(i) for i in batch_mvp_idx]
        if idx and all(idx[k + 1] == idx[k] + 1 for k in range(len(idx) - 1)) and 0 <= idx[0] and idx[-1] < t.shape[0]:
            return t[idx[0]:idx[0] + len(idx)]
        return t[idx]

    def select_rays(self, batch_mvp_idx, batch_patch_min, patch_width, patch_height, _origins=None):
        """Rays of the (patch_height, patch_width) window at patch_min of each batch item (reference :264-302).
        ``_origins``: the (B,2) origins as a list, where the caller has read them back already (``_window``)."""
        # one read-back of the (B,2) patch origins serves the reference's two bound checks (same messages) and tells whether
        # every window is the whole frame -- then the ray tensors are handed over as views, not gathered into a copy
        # (2 x 24.9 MB per camera at 1080p)
        pm = _origins if _origins is not None else [[int(v) for v in row] for row in batch_patch_min.tolist()]
        assert all(p[0] + patch_width <= self.width for p in pm), "Some b_patch_max_x exceed self.width"
        assert all(p[1] + patch_height <= self.height for p in pm), "Some b_patch_max_y exceed self.height"
        if patch_width == self.width and patch_height == self.height and all(p[0] == 0 and p[1] == 0 for p in pm):
            return self._camera_rows(self.ray_o, batch_mvp_idx), self._camera_rows(self.ray_d, batch_mvp_idx)
        px0 = batch_patch_min[:, 0].long()
        py0 = batch_patch_min[:, 1].long()
        dev = self.ray_o.device
        cams = torch.as_tensor(list(batch_mvp_idx), device=dev, dtype=torch.long)
        rows = py0.to(dev).view(-1, 1, 1) + torch.arange(patch_height, device=dev).view(1, -1, 1)
        cols = px0.to(dev).view(-1, 1, 1) + torch.arange(patch_width, device=dev).view(1, 1, -1)
        cam = cams.view(-1, 1, 1)
        return self.ray_o[cam, rows, cols], self.ray_d[cam, rows, cols]

    # -- windows on the deferred path ------------------------------------------------
    def _window(self, batch_mvp_idx, patch_min, patch_width, patch_height, device):
        """The checks of a window of rasterize / generate / coverage / render -> ``_Window`` (patch_min as (B,2) int32 on
        ``device``, the origins as a list, the size): the origins are read back once, for all checks (and for ``select_rays``).
        ValueError for a shape other than (B,2), a negative size or a negative origin; ``select_rays``' two assertions for a
        window past the frame."""
        B = len(batch_mvp_idx)
        if patch_min.dim() != 2 or tuple(patch_min.shape) != (B, 2):
            raise ValueError(f"patch_min must have dimensions ({B}, 2), got {tuple(patch_min.shape)}")
        patch_width, patch_height = int(patch_width), int(patch_height)
        if patch_width < 0 or patch_height < 0:
            raise ValueError("patch_width and patch_height must not be negative")
        pm = [[int(v) for v in row] for row in patch_min.tolist()]
        if any(p[0] < 0 or p[1] < 0 for p in pm):
            raise ValueError("patch_min must not be negative")
        assert all(p[0] + patch_width <= self.width for p in pm), "Some b_patch_max_x exceed self.width"
        assert all(p[1] + patch_height <= self.height for p in pm), "Some b_patch_max_y exceed self.height"
        return _Window(patch_min.to(device=device, dtype=torch.int32).contiguous(), pm, patch_width, patch_height)

    def _sized_window(self, batch_mvp_idx, patch_min, patch_width, patch_height, device):
        """The window of rasterize / generate, which take it as ``patch_min`` with both sizes or not at all -> ``_window``'s, or
        None: the full frame."""
        if patch_min is None:
            if patch_width is not None or patch_height is not None:
                raise ValueError("patch_width / patch_height need patch_min")
            return None
        if patch_width is None or patch_height is None:
            raise ValueError("patch_min needs patch_width and patch_height")
        return self._window(batch_mvp_idx, patch_min, patch_width, patch_height, device)

    def _layers_window(self, batch_mvp_idx, render_layers, patch_min, device, check_frame):
        """The window of the ops that are handed ``render_layers`` (B,H,W,L), a window's with ``patch_min`` (its H, W are the
        window's size) -> ``_window``'s, or None: the full frame.  ``check_frame``: without ``patch_min``, render_layers must
        have that rank and the frame's size (bary_derivatives, shading_vectors; coverage and render leave both to the op)."""
        if patch_min is None and not check_frame:
            return None
        if render_layers.dim() != 4:
            raise ValueError(f"render_layers must have dimensions (B, H, W, L), got {tuple(render_layers.shape)}")
        if patch_min is not None:
            return self._window(batch_mvp_idx, patch_min, render_layers.shape[2], render_layers.shape[1], device)
        if tuple(render_layers.shape[1:3]) != (self.height, self.width):
            raise ValueError(f"render_layers must cover the {self.width} x {self.height} frame (or come with patch_min), "
                             f"got {tuple(render_layers.shape)}")
        return None

    def _entered(self, window):
        """The context of a call on ``window`` (None: the full frame, no window) that takes no rays."""
        return _C.window(None if window is None else window.patch_min, self.width, self.height)

    def _analytic(self):
        return getattr(self, "analytic_rays", False)

    def _ray_cam_rows(self, batch_mvp_idx):
        """inv(mv), inv(proj) of the selected views, (B,32): rows of the block analytic rays keep, or built here."""
        if self._analytic():
            return self.ray_cam[torch.as_tensor(list(batch_mvp_idx), device=self.ray_cam.device, dtype=torch.long)]
        idx = list(batch_mvp_idx)
        with torch.no_grad():
            return torch.cat((torch.inverse(self.mv[idx]).reshape(-1, 16), torch.inverse(self.proj[idx]).reshape(-1, 16)), dim=1)

    def _rays(self, batch_mvp_idx, window=None, patch=None):
        """(ray_o, ray_d, context) of a call on the selected views: the ray tensors' rows (views, for consecutive cameras), or
        placeholders that are never read under analytic rays, whose cameras the context carries to the op.  ``window``
        (``_window``'s): the window's cut, and the context carries the origins too (``_C.window``).  ``patch`` =
        (batch_patch_min, patch_width, patch_height): ``forward``'s, the reference's route -- the cut, but the origins are
        an argument of the op, not the context's."""
        f32 = torch.float32
        ctx = [] if window is None else [self._entered(window)]
        if self._analytic():
            cam = self._ray_cam_rows(batch_mvp_idx)
            ph = torch.empty((cam.shape[0], 0, 0, 3), dtype=f32, device=cam.device)
            return ph, ph, _Entered(*ctx, _C.analytic_rays(cam.contiguous(), self.width, self.height))
        if window is not None:
            ray_o, ray_d = self.select_rays(batch_mvp_idx, window.patch_min, window.width, window.height, _origins=window.origins)
        elif patch is not None:
            ray_o, ray_d = self.select_rays(batch_mvp_idx, *patch)
        else:
            ray_o, ray_d = self._camera_rows(self.ray_o, batch_mvp_idx), self._camera_rows(self.ray_d, batch_mvp_idx)
        return ray_o.to(f32), ray_d.to(f32), _Entered(*ctx) if ctx else contextlib.nullcontext()      # (nothing to enter: the full frame)

    # -- projection --------------------------------------------------------------
    def compute_verts_ndc_image(self, verts, mv, proj):
        """verts (P,3) -> verts_ndc (B,P,3), verts_image (B,P,2) in full-image pixel units (reference :239-262)."""
        hom = torch.cat((verts, torch.ones_like(verts[:, :1])), dim=-1)      # (P,4)
        clip = torch.matmul(torch.matmul(hom, mv.transpose(1, 2)), proj.transpose(1, 2))   # (B,P,4)
        w = clip[..., 3:4]
        w = torch.where((w >= 0.0) & (w < _W_EPS), torch.full_like(w, _W_EPS), w)
        w = torch.where((w < 0.0) & (w > -_W_EPS), torch.full_like(w, -_W_EPS), w)
        ndc = clip[..., :3] / w
        half = (ndc[..., :2] + 1) * 0.5
        image = torch.stack((half[..., 0] * self.width, half[..., 1] * self.height), dim=-1)
        return ndc, image

    def _project(self, batch_mvp_idx, verts, faces, graph):
        """verts_ndc (B,P,3), verts_image (B,P,2) of the selected views: the fused projection on GPU tensors, else
        ``compute_verts_ndc_image``.  ``graph`` False: without an autograd graph -- the plan's bins and depth cull, constants
        of the op like the rays."""
        mv = self.mv[batch_mvp_idx]
        proj = self.proj[batch_mvp_idx]
        i32, f32 = torch.int32, torch.float32
        with contextlib.nullcontext() if graph else torch.no_grad():
            if getattr(self, "fused_prep", False) and verts.is_cuda:
                from . import prep
                return prep.project(verts.to(f32), faces.to(i32), mv.to(f32), proj.to(f32), self.width, self.height)
            return self.compute_verts_ndc_image(verts, mv, proj)

    # -- forward -----------------------------------------------------------------
    def forward(self, batch_mvp_idx: List[int], batch_patch_min: torch.Tensor, patch_width: int,
                patch_height: int, verts: torch.Tensor, faces: torch.Tensor, verts_color: torch.Tensor,
                faces_opacity: torch.Tensor, faces_intense: torch.Tensor, background: torch.Tensor,
                aa_temperature: float = 1.0, return_alpha: bool = False, return_face_weights: bool = False):
        """Render ``len(batch_mvp_idx)`` patches; returns color (B,H,W,3), depth (B,H,W) in [0,1] (0 = background).

        Not in the reference's signature: ``return_alpha=True`` returns (color, depth, alpha), alpha (B,H,W) = 1 - T, the
        T the colour multiplied the background by -- differentiable w.r.t. faces_opacity and, through the AA coverage,
        verts.  ``return_face_weights=True`` appends face_weights (B,F) float32: for each view and face, the sum over the
        patch's pixels of alpha * T of the face's blends, the factor its colour gets in C += c alpha T (sum_f equals the
        alpha image's sum; > 0 marks the faces the view used).  Not differentiable; also under torch.no_grad().  Float
        atomics: the last bits may vary from run to run."""
        ray_o, ray_d, ctx = self._rays(batch_mvp_idx, patch=(batch_patch_min, patch_width, patch_height))
        with ctx, _C.alpha_output(return_alpha), _C.face_weights_output(return_face_weights):
            return self._forward_with_rays(batch_mvp_idx, ray_o, ray_d, batch_patch_min, patch_width, patch_height, verts, faces,
                                           verts_color, faces_opacity, faces_intense, background, aa_temperature)

    def rasterize(self, batch_mvp_idx: Sequence[int], verts: torch.Tensor, faces: torch.Tensor, num_layers: int,
                  faces_existence: torch.Tensor = None, patch_min: torch.Tensor = None, patch_width: int = None,
                  patch_height: int = None, overlap: bool = False):
        """The first ``num_layers`` faces each pixel's ray hits, over the full frame of every selected view or over a window of
        it (not in the reference) -> render_layers (B,H,W,L) int32 face ids (-1 = empty), render_layers_cnt (B,H,W) int32, bary (B,H,W,L,3)
        float32 = the weights of faces[f][0..2] at the hit (perspective-correct), t (B,H,W,L) float32 = the hit's distance
        along the pixel's ray; -1 in every empty slot.

        Candidates are the faces whose image bbox touches the pixel's 16x16 tile and whose NDC depth range meets [-1, 1]
        (``faces_existence`` == 0 drops a face; None keeps all); a hit is the pixel's ray meeting the triangle (t >= 0,
        barycentrics >= 0); hits are ordered by (t, face id).  render_layers can go straight to ``LayeredRenderer.render``.
        bary and t are differentiable w.r.t. ``verts`` (``RasterizeFunction``); nothing flows through the rays (cameras get
        no gradient here) or through which faces are listed.  ``interpolate`` turns the ids and bary into an image of any
        per-vertex attribute (normals, UVs, features), differentiably.

        Window: ``patch_min`` (B,2) int32 (x, y) per selected view, ``patch_width``, ``patch_height`` -- ``forward``'s
        ``batch_patch_min`` and sizes -- rasterize that window of each view only: H, W above are then patch_height, patch_width.
        Window pixel (x, y) of view b is frame pixel (x + patch_min[b,0], y + patch_min[b,1]) and takes that pixel's ray; the
        16x16 tiles (the candidates' bbox test) are anchored at the window's origin, as in ``forward``.  So a window equals the
        crop of the full frame where its origin is a multiple of 16, and elsewhere may differ in hits of faces whose bbox
        misses the pixel's tile in one of the two grids.  The window must lie inside the frame (``select_rays``' assertions;
        ValueError for a negative origin, or for ``patch_min`` without a size); an empty window returns empty tensors and
        launches nothing.  Without ``patch_min`` the sizes must be None as well.

        ``overlap=True`` -> (render_layers, render_layers_cnt, bary, t, inside): the faces ``forward`` blends at a temperature
        > 0, so that the deferred path draws a silhouette as ``forward`` does.  Of the same candidates a face is listed where
        its projected triangle overlaps the pixel's square [X, X+1] x [Y, Y+1] (frame coordinates) with non-zero area by
        ``coverage``'s clipper, the ray meets its plane (not in the plane itself) and the slot's t >= 0.  bary is the ray's
        barycentrics clamped onto the triangle (``clamp_bary_uv``), inside (B,H,W,L) bool tells the slots where the ray hits
        the face itself (nothing was clamped): those are exactly the standard mode's hits, t included.  Elsewhere t is the ray
        parameter of the clamped point's projection onto the ray, continuous across the triangle's edge.  Order (t, face
        id); empty slots hold -1, and False in inside.  Hand ``inside`` to ``coverage`` so that a grazing face mixes as it
        does in ``forward``.  Differentiable in bary and t w.r.t. ``verts`` through the clamp (``RasterizeOverlapFunction``)."""
        fn = RasterizeOverlapFunction if overlap else RasterizeFunction
        window = self._sized_window(batch_mvp_idx, patch_min, patch_width, patch_height, verts.device)
        pw, ph = (self.width, self.height) if window is None else (window.width, window.height)
        i32, f32 = torch.int32, torch.float32
        B, L, dev = len(batch_mvp_idx), int(num_layers), verts.device
        if window is not None and window.empty:
            out = (torch.empty((B, ph, pw, L), dtype=i32, device=dev), torch.empty((B, ph, pw), dtype=i32, device=dev),
                   torch.empty((B, ph, pw, L, 3), dtype=f32, device=dev), torch.empty((B, ph, pw, L), dtype=f32, device=dev))
            if overlap:
                out += (torch.empty((B, ph, pw, L), dtype=torch.bool, device=dev),)
            return out
        verts_ndc, verts_image = self._project(batch_mvp_idx, verts, faces, graph=False)
        fe = None if faces_existence is None else faces_existence.to(i32)
        ray_o, ray_d, ctx = self._rays(batch_mvp_idx, window)
        with ctx:
            return fn.apply(verts.to(f32), faces.to(i32), fe, verts_ndc.to(f32), verts_image.to(f32), ray_o, ray_d, pw, ph, L)

    def interpolate(self, render_layers: torch.Tensor, bary: torch.Tensor, attr: torch.Tensor, attr_faces: torch.Tensor):
        """Attribute images from ``rasterize``'s hits (not in the reference): render_layers (B,H,W,L) int32 face ids (as
        ``rasterize`` / ``generate`` return them, or hand-built), bary (B,H,W,L,3) float32 weights of attr_faces[f][0..2],
        attr (N,C) float32 shared by the views or (B,N,C) one table per view (any C >= 1), attr_faces (F,3) int32 rows of
        attr (the mesh's ``faces`` for per-vertex data, or a table of its own, e.g. across UV seams) -> out (B,H,W,L,C)
        float32 = (bary0 attr[v0] + bary1 attr[v1]) + bary2 attr[v2] per slot.

        A slot whose id is outside [0, F), or whose attr_faces row names a row outside [0, N), is empty: zeros out, whatever
        its bary holds, and no gradient.  Differentiable w.r.t. ``attr`` and ``bary`` (``InterpolateFunction``); through
        ``bary``, ``rasterize``'s backward carries the gradient on to ``verts``."""
        i32, f32 = torch.int32, torch.float32
        return InterpolateFunction.apply(render_layers.to(i32), bary.to(f32), attr.to(f32), attr_faces.to(i32))

    def texture(self, uv: torch.Tensor, tex: torch.Tensor, render_layers: torch.Tensor = None, filter_mode: str = "linear",
                boundary_mode: str = "wrap", uv_da: torch.Tensor = None, mip: torch.Tensor = None, max_mip_level: int = None,
                mip_level: torch.Tensor = None):
        """A texture sampled at ``interpolate``'s UVs (not in the reference): uv (B,H,W,L,2) float32 = (u, v), u along the
        texture's width (what ``interpolate`` returns for a 2-channel attribute), tex (Ht,Wt,C) float32 shared by the views or
        (B,Ht,Wt,C) one texture per view, channel-last, any C >= 1, render_layers (B,H,W,L) int32 or None -> out (B,H,W,L,C)
        float32.  Texel centres sit at ((i + 0.5) / Wt, (j + 0.5) / Ht); ``filter_mode`` "linear" (bilinear), "nearest" or
        "linear-mipmap-linear" (trilinear, below), ``boundary_mode`` "wrap" (repeat) or "clamp".

        A slot with ``render_layers`` < 0 (None: no slot, by id), or whose uv is not finite, is empty: zeros out, nothing
        read from the texture through it, no gradient.  Differentiable w.r.t. ``tex`` and ``uv`` (``TextureFunction``); through
        ``uv``, ``interpolate``'s and ``rasterize``'s backwards carry the gradient on to the UV table and to ``verts``.

        ``filter_mode="linear-mipmap-linear"`` needs ``uv_da`` (B,H,W,L,4) float32 = (du/dX, dv/dX, du/dY, dv/dY), the UV
        footprint of each slot's pixel: ``torch.cat([interpolate(render_layers, dbary_dx, uv_table, uv_faces),
        interpolate(render_layers, dbary_dy, uv_table, uv_faces)], -1)`` of ``bary_derivatives``' outputs.  With r2 = the larger
        squared length of the two footprint vectors in texels, the level of detail is 0.5 log2(r2) with the mantissa taken
        linearly (0 where r2 <= 1: at most 0.043 levels below the exact logarithm, include/dm2_hip.h), and the slot blends the
        bilinear samples of the two levels of ``texture_mipmaps``' chain round it; at or below level 0 the result is
        "linear"'s, to the bit, beyond the last level the last level's.  ``mip``: that chain for ``tex`` and ``max_mip_level``
        (RuntimeError where its shape does not match them); None builds it here, so that the texture's gradient flows through
        ``MipmapFunction``.  A slot whose ``uv_da`` is not finite is empty as well.  Differentiable w.r.t. ``tex``, ``mip`` and
        ``uv`` (``TextureMipFunction``); ``uv_da`` gets no gradient: the level of detail is a constant of the op.  ValueError
        for the mode without ``uv_da``, and for ``uv_da`` or ``mip`` with another mode.

        ``boundary_mode="cube"`` looks a cube map up by direction: ``uv`` is then (B,H,W,L,3) float32, a direction per slot
        of any non-zero length (``interpolate``'s output for per-vertex normals, normalised or not; a reflected view vector),
        ``tex`` (6,N,N,C) shared by the views or (B,6,N,N,C), square faces in the order +x, -x, +y, -y, +z, -z with OpenGL's
        face coordinates (nvdiffrast's layout).  The component of largest magnitude picks the face (x before y before z on
        ties); ``filter_mode`` "linear" takes its taps beyond a face's border from the adjacent face, and at a cube corner,
        where one of the four taps does not exist, blends the other three with their weights renormalised, so the lookup is
        continuous over the whole sphere; "nearest" takes the face's nearest texel.  A slot with a negative id, a non-finite
        component or an all-zero direction is empty.  Differentiable w.r.t. ``tex`` and the direction
        (``TextureCubeFunction``); the direction's gradient is orthogonal to it.  ValueError naming ``boundary_mode`` for
        "linear-mipmap-linear", ``mip`` or ``max_mip_level`` with "cube" and without ``mip_level``, and for ``uv_da`` with
        "cube" always: a cube has no footprint-driven level.

        ``filter_mode="linear-mipmap-linear"`` with ``boundary_mode="cube"`` and ``mip_level`` (B,H,W,L) float32 samples the
        cube's mip chain at a level of detail per slot (a glossy reflection: the level from the roughness): level 0 is
        ``tex``, level k has faces of N >> k texels and exists while N >> (k - 1) is even and k <= ``max_mip_level``.  ``mip``
        (6,T,C) or (B,6,T,C) holds, per face, levels 1 .. nlev-1 packed as ``_C.mip_layout(N, N, max_mip_level)`` lays them
        out; None builds the box chain here (``texture_mipmaps``), so that ``tex.grad`` receives both the direct gradient and
        the chain's; a chain the caller supplies (prefiltered, or learned) gets its own gradient and need not be the box
        chain.  At or below level 0 the result is "linear"'s to the bit, at or beyond the last level the last level's, in
        between c_j + f (c_{j+1} - c_j) of the two levels' cube samples (seams and corners at each level's own size).  A
        slot whose level is not finite is empty as well.  Differentiable w.r.t. ``tex``, ``mip``, the direction and
        ``mip_level`` (``TextureCubeMipFunction``): dL/dmip_level = g . (c_{j+1} - c_j) between two levels, 0 where the level
        is clamped.  ValueError naming ``mip_level`` for ``mip_level`` with any other combination of modes."""
        i32, f32 = torch.int32, torch.float32
        rl = None if render_layers is None else render_layers.to(i32)
        if boundary_mode == "cube" and mip_level is not None:
            if uv_da is not None:
                raise ValueError('boundary_mode "cube" takes no uv_da: the level of detail comes in through mip_level')
            if filter_mode != "linear-mipmap-linear":
                raise ValueError('mip_level belongs to filter_mode "linear-mipmap-linear" with boundary_mode "cube"')
            tex = tex.to(f32)
            if mip is None:
                mip = self.texture_mipmaps(tex, max_mip_level)
            return TextureCubeMipFunction.apply(uv.to(f32), mip_level.to(f32), tex, mip.to(f32), rl, max_mip_level)
        if mip_level is not None:
            raise ValueError('mip_level belongs to filter_mode "linear-mipmap-linear" with boundary_mode "cube"')
        if boundary_mode == "cube":
            if filter_mode == "linear-mipmap-linear" or uv_da is not None or mip is not None or max_mip_level is not None:
                raise ValueError('boundary_mode "cube" takes filter_mode "linear" or "nearest" and no uv_da, mip or max_mip_level; '
                                 '"linear-mipmap-linear" with mip_level samples the cube\'s mip chain')
            return TextureCubeFunction.apply(uv.to(f32), tex.to(f32), rl, filter_mode)
        if filter_mode == "linear-mipmap-linear":
            if uv_da is None:
                raise ValueError('filter_mode "linear-mipmap-linear" needs uv_da')
            tex = tex.to(f32)
            if mip is None:
                mip = MipmapFunction.apply(tex, max_mip_level)
            return TextureMipFunction.apply(uv.to(f32), uv_da.to(f32), tex, mip.to(f32), rl, boundary_mode, max_mip_level)
        if uv_da is not None or mip is not None:
            raise ValueError('uv_da and mip belong to filter_mode "linear-mipmap-linear"')
        return TextureFunction.apply(uv.to(f32), tex.to(f32), rl, filter_mode, boundary_mode)

    def texture3d(self, xyz: torch.Tensor, grid: torch.Tensor, render_layers: torch.Tensor = None, filter_mode: str = "linear",
                  boundary_mode: str = "clamp"):
        """A voxel grid looked up at per-slot positions (not in the reference): an appearance field over space, which needs no
        UV table and so follows a mesh whose connectivity changes.  xyz (B,H,W,L,3) float32 = the position in the grid's unit
        cube, x along the grid's last spatial axis and z along its first (``(position - lo) / (hi - lo)`` of
        ``shading_vectors``' position for a grid over the box [lo, hi]), grid (N,N,N,C) float32 shared by the views or
        (B,N,N,N,C) one grid per view, channel-last, indexed [k][j][i], any C >= 1, render_layers (B,H,W,L) int32 or None
        -> out (B,H,W,L,C) float32.  Voxel centres sit at ((i + 0.5) / N, (j + 0.5) / N, (k + 0.5) / N); ``filter_mode``
        "linear" (trilinear) or "nearest", ``boundary_mode`` "clamp" or "wrap" (repeat).

        A slot with ``render_layers`` < 0 (None: no slot, by id), or with a coordinate that is not finite, is empty: zeros
        out, nothing read from the grid through it (the zeros ``shading_vectors`` writes into its empty slots never reach voxel
        (0, 0, 0)), no gradient.  Differentiable w.r.t. ``grid`` and ``xyz`` (``TextureVolumeFunction``); through ``xyz``,
        ``shading_vectors``' and ``rasterize``'s backwards carry the gradient on to ``verts``.  ValueError for an unknown
        mode."""
        if filter_mode not in _C.TEX_FILTERS:
            raise ValueError(f"filter_mode must be one of {sorted(_C.TEX_FILTERS)}, got {filter_mode!r}")
        if boundary_mode not in _C.TEX_BOUNDARIES:
            raise ValueError(f"boundary_mode must be one of {sorted(_C.TEX_BOUNDARIES)}, got {boundary_mode!r}")
        i32, f32 = torch.int32, torch.float32
        rl = None if render_layers is None else render_layers.to(i32)
        return TextureVolumeFunction.apply(xyz.to(f32), grid.to(f32), rl, filter_mode, boundary_mode)

    def hash_grid(self, xyz: torch.Tensor, table: torch.Tensor, render_layers: torch.Tensor = None, base_resolution: int = 16,
                  growth: float = 1.5, filter_mode: str = "linear", boundary_mode: str = "clamp"):
        """A multiresolution hash encoding looked up at per-slot positions (not in the reference): the input of a small MLP
        that models appearance over space at a detail no dense grid can hold.  xyz (B,H,W,L,3) float32 = the position in the
        field's unit cube, axes and meaning as for ``texture3d``; table (NL,T,F) float32 shared by the views: NL = 1..32
        levels, T = 2^4..2^24 rows per level, F = 1, 2, 4 or 8 features per row; render_layers (B,H,W,L) int32 or None
        -> out (B,H,W,L,NL*F) float32, the levels' samples concatenated, channel l * F + f.

        Level l is ``texture3d``'s lookup (``filter_mode`` "linear" or "nearest", ``boundary_mode`` "clamp" or "wrap") of a
        virtual R_l^3 grid, ``hash_grid_resolutions(NL, base_resolution, growth)``: R_0 = base_resolution,
        R_{l+1} = (R_l * 16 growth) >> 4, ``growth`` a multiple of 1/16 from 1.0625 to 2.  Its voxel (k, j, i) is row
        (k R_l + j) R_l + i of table[l] while R_l^3 <= T and row (i ^ j * 2654435761 ^ k * 805459861) mod T after that.

        A slot with ``render_layers`` < 0 (None: no slot, by id), or with a coordinate that is not finite, is empty: zeros
        out, nothing read from the table through it, no gradient.  Differentiable w.r.t. ``table`` and ``xyz``
        (``HashGridFunction``); through ``xyz``, ``shading_vectors``' and ``rasterize``'s backwards carry the gradient on to
        ``verts``.  ValueError for an unknown mode, a bad ``growth`` or ``base_resolution``, or a table whose T or F the op
        does not take."""
        if filter_mode not in _C.TEX_FILTERS:
            raise ValueError(f"filter_mode must be one of {sorted(_C.TEX_FILTERS)}, got {filter_mode!r}")
        if boundary_mode not in _C.TEX_BOUNDARIES:
            raise ValueError(f"boundary_mode must be one of {sorted(_C.TEX_BOUNDARIES)}, got {boundary_mode!r}")
        if table.dim() != 3:
            raise ValueError(f"table must have dimensions (NL, T, F), got {tuple(table.shape)}")
        NL, T, F = (int(x) for x in table.shape)
        lo, hi = _C.HASH_GRID_LOG2_ROWS
        if T < 1 or T & (T - 1) or not lo <= T.bit_length() - 1 <= hi:
            raise ValueError(f"table: T must be a power of two from 2^{lo} to 2^{hi} rows per level, got {T}")
        if F not in _C.HASH_GRID_FEATURES:
            raise ValueError(f"table: F must be 1, 2, 4 or 8 features per row, got {F}")
        _C.hash_grid_resolutions(NL, base_resolution, growth)            # (ValueError for growth, NL, base_resolution, R_{NL-1})
        i32, f32 = torch.int32, torch.float32
        rl = None if render_layers is None else render_layers.to(i32)
        return HashGridFunction.apply(xyz.to(f32), table.to(f32), rl, int(base_resolution), float(growth), filter_mode, boundary_mode)

    @staticmethod
    def hash_grid_resolutions(num_levels: int, base_resolution: int = 16, growth: float = 1.5):
        """[R_0, ..., R_{NL-1}] of ``hash_grid``: R_0 = base_resolution, R_{l+1} = (R_l * 16 growth) >> 4."""
        return _C.hash_grid_resolutions(num_levels, base_resolution, growth)

    def texture_mipmaps(self, tex: torch.Tensor, max_mip_level: int = None):
        """The mip chain of a texture (not in the reference): tex (Ht,Wt,C) float32 or (B,Ht,Wt,C) -> mip (T,C) or (B,T,C)
        float32.  Level 0 is ``tex`` itself and is not copied; level k+1 exists while both extents of level k are even and
        k < ``max_mip_level`` (None: no limit), has half the extents, and each of its texels is the mean of its 2 x 2 parents,
        ((p00 + p10) + (p01 + p11)) * 0.25.  ``mip`` holds levels 1 .. nlev-1 one after the other, each (H_k, W_k, C)
        row-major (``_C.mip_layout``); T = 0 when no level can be built (an odd extent).  Differentiable w.r.t. ``tex``
        (``MipmapFunction``): the backward is a gather, deterministic.

        A cube map (6,N,N,C) is six textures and gives (6,T,C); a cube per view (B,6,N,N,C) gives (B,6,T,C).  The 2 x 2 mean
        within each face is the cube's box chain (a texel's parents never lie on another face), which is what
        ``texture(..., "linear-mipmap-linear", "cube", mip_level=...)`` builds when it is given no ``mip``."""
        tex = tex.to(torch.float32)
        if tex.dim() == 5:
            mip = MipmapFunction.apply(tex.reshape((-1,) + tuple(tex.shape[2:])), max_mip_level)
            return mip.reshape(tuple(tex.shape[:2]) + tuple(mip.shape[1:]))
        return MipmapFunction.apply(tex, max_mip_level)

    @staticmethod
    def cube_prefilter_norm(N: int, max_mip_level: int = None, device=None):
        """The normalisation of ``cube_prefilter`` for cubes with faces of N x N under ``max_mip_level`` -> norm (6,T) float32:
        per chain texel the lobe's weight sum W[o] = sum_s K(o,s) Om_s (the filter applied to a chain of ones).  It depends on
        (N, max_mip_level) alone: build it once per cube size and pass it as ``cube_prefilter(..., norm=norm)``.  Nothing is
        cached here."""
        T = _C.mip_layout(N, N, max_mip_level)[2]
        ones = torch.ones((6, T, 1), dtype=torch.float32, device=torch.device("cuda") if device is None else device)
        return _C.cube_prefilter_cuda(ones, N, max_mip_level).reshape(6, T)

    def cube_prefilter(self, tex: torch.Tensor, max_mip_level: int = None, norm: torch.Tensor = None):
        """A cube map's roughness chain (not in the reference): tex (6,N,N,C) float32 or (B,6,N,N,C) -> mip (6,T,C) or
        (B,6,T,C) float32 in ``_C.mip_layout(N, N, max_mip_level)``'s packing, ready for ``texture(dirs, tex, rl,
        "linear-mipmap-linear", "cube", mip=mip, max_mip_level=max_mip_level, mip_level=roughness * (nlev - 1))``.

        Level k >= 1 of nlev levels is level k of the box chain (``texture_mipmaps``) convolved over the whole sphere, across
        the faces, with the GGX lobe of roughness r = k / (nlev - 1) (a = r^2; the split-sum lobe D(n.h) (n.l) with n = v = r,
        weighted by each texel's solid angle) and divided by the lobe's weight sum ``norm``: a constant cube stays constant.
        Level 0, the mirror, is ``tex`` itself.  The lobe is cut where it has fallen below 1/4096 of its peak (at most 1/64 of
        its mass; only below r = 0.298); at r = 1 it is the cosine lobe, so the last level of a full chain is the diffuse
        irradiance map over pi.  The contract is in include/dm2_hip.h under dm2_cube_prefilter.

        ``norm``: ``cube_prefilter_norm(N, max_mip_level)``, (6,T); None builds it in this call.  An odd N gives T = 0 and an
        empty chain.  Differentiable w.r.t. ``tex`` (``CubePrefilterFunction`` on top of ``MipmapFunction``): the backward is
        the filter's transpose, a gather like the forward, so both are deterministic and free of float atomics."""
        tex = tex.to(torch.float32)
        if tex.dim() not in (4, 5) or tex.shape[-4] != 6 or tex.shape[-3] != tex.shape[-2]:
            raise RuntimeError(f"cube_prefilter: tex must have dimensions (6, N, N, C) or (B, 6, N, N, C), got {tuple(tex.shape)}")
        N = int(tex.shape[-2])
        T = _C.mip_layout(N, N, max_mip_level)[2]
        if norm is None:
            norm = Renderer.cube_prefilter_norm(N, max_mip_level, tex.device)
        elif tuple(norm.shape) != (6, T):
            raise RuntimeError(f"cube_prefilter: norm must have dimensions {(6, T)} for N {N} and max_mip_level {max_mip_level}, "
                               f"got {tuple(norm.shape)}")
        chain = Renderer.texture_mipmaps(self, tex, max_mip_level)
        return CubePrefilterFunction.apply(chain, N, max_mip_level) / norm.to(torch.float32).unsqueeze(-1)

    def bary_derivatives(self, batch_mvp_idx: Sequence[int], render_layers: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor,
                         patch_min: torch.Tensor = None):
        """The footprint of a pixel on each listed face (not in the reference): render_layers (B,H,W,L) int32 face ids (as
        ``rasterize`` returns them, or hand-built), verts (P,3), faces (F,3) -> (dbary_dx, dbary_dy), each (B,H,W,L,3)
        float32: the derivatives of the slot's perspective-correct barycentrics (``rasterize``'s bary, unclamped) with respect
        to the pixel's x and y position in pixels.  Each goes into ``interpolate`` as its ``bary``: ``interpolate`` is linear
        in ``bary``, so ``interpolate(render_layers, dbary_dx, uv_table, uv_faces)`` is (du/dX, dv/dX).

        Computed from the cameras' inv(mv), inv(proj) (the block ``Renderer(analytic_rays=True)`` keeps; a Renderer with ray
        tensors builds the selected views' rows here) and the vertices: neither the ray tensors nor ``bary`` are read.  A slot
        whose id is outside [0, F), or whose face names a vertex outside [0, P), is empty: zeros; zeros too where the ray
        lies in the face's plane.  Not differentiable (``BaryDerivativesFunction`` marks both outputs so): the footprint is
        a constant of the pipeline, as nothing flows through which faces are listed.

        Window: with ``patch_min`` (B,2) int32, render_layers is a window's and slot (b, y, x) is frame pixel
        (x + patch_min[b,0], y + patch_min[b,1]): the crop of the full-frame result.  Checks and errors are ``coverage``'s; an
        empty window launches nothing."""
        i32, f32 = torch.int32, torch.float32
        window = self._layers_window(batch_mvp_idx, render_layers, patch_min, verts.device, check_frame=True)
        if render_layers.numel() == 0:
            z = torch.empty(tuple(render_layers.shape) + (3,), dtype=f32, device=verts.device)
            return z, z.clone()
        cam = self._ray_cam_rows(batch_mvp_idx).to(device=verts.device, dtype=f32).contiguous()
        with self._entered(window):
            return BaryDerivativesFunction.apply(render_layers.to(i32), verts.to(f32), faces.to(i32), cam)

    def composite(self, values: torch.Tensor, alpha: torch.Tensor, render_layers: torch.Tensor = None,
                  background: torch.Tensor = None):
        """Shaded layers blended front to back into an image (not in the reference): values (B,H,W,L,C) float32, any C >= 1
        (what ``interpolate`` or ``texture`` return, or anything computed from them), alpha (B,H,W,L) float32, one opacity per
        slot, or (F,) float32, one per face (``faces_opacity``; gathered as alpha[render_layers] inside the op, which then
        needs ``render_layers``), render_layers (B,H,W,L) int32 or None, background (C,) float32 or None (no background term)
        -> out (B,H,W,C) float32, acc (B,H,W) float32 = 1 - T (the alpha image of ``return_alpha``).

        ``LayeredRenderer.render``'s blend with the colour supplied by the caller: per pixel, from T = 1, every non-empty
        slot adds values * (a * T) and multiplies T by 1 - a, until T < 1e-4; out = the sum + T * background.  A slot with a
        negative id (per-face alpha: an id outside [0, F)) is empty: neither its values nor its alpha are looked at.  alpha is
        used as it stands (no clamp).  Differentiable w.r.t. ``values`` and ``alpha`` (``CompositeFunction``); ``background``
        gets no gradient, and nothing flows through which slots are listed."""
        i32, f32 = torch.int32, torch.float32
        rl = None if render_layers is None else render_layers.to(i32)
        bg = None if background is None else background.to(f32)
        return CompositeFunction.apply(values.to(f32), alpha.to(f32), rl, bg)

    def coverage(self, batch_mvp_idx: Sequence[int], render_layers: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor,
                 temperature: float = 1.0, patch_min: torch.Tensor = None, inside: torch.Tensor = None):
        """The analytic pixel coverage of the listed faces (not in the reference): render_layers (B,H,W,L) int32 face ids over
        the full frame (as ``rasterize`` / ``generate`` return them, or hand-built), verts (P,3), faces (F,3), temperature in
        [0, 1] (ValueError otherwise) -> cov (B,H,W,L) float32, ``Renderer.forward``'s coverage ratio of a hit:
        (1 - temperature) + area * temperature, area the overlap of the projected triangle with the pixel [x, x+1] x [y, y+1].
        ``composite(values, faces_opacity[render_layers.clamp(min=0).long()] * cov, render_layers, background)`` then blends
        anti-aliased layers, and a mask or silhouette loss moves ``verts``.

        A slot whose id is outside [0, F), or whose face names a vertex outside [0, P), is empty: cov = 0.  Where the triangle
        misses the pixel (or the clipper reports an error) cov = 0 too; at temperature 0 cov = 1 in every non-empty slot.
        Whether the pixel's ray hits the face is not looked at.  Differentiable w.r.t. ``verts`` and, where they require grad,
        the cameras, through the projection (``CoverageFunction``); nothing flows through which faces are listed.

        Window: with ``patch_min`` (B,2) int32 (x, y) per selected view, render_layers is a window's (as ``rasterize`` /
        ``generate`` return it for the same ``patch_min``; its own H, W are the window's size) and the pixel of slot (b, y, x)
        is [x + patch_min[b,0], ...+1] x [y + patch_min[b,1], ...+1] of the frame: the crop of the full-frame result.  The
        window must lie inside the frame (``select_rays``' assertions; ValueError for a negative origin).

        ``inside`` (B,H,W,L) bool or integer, ``rasterize(overlap=True)``'s: a non-empty slot where it is 0 lists a face that
        only grazes the pixel and mixes as ``forward`` mixes such a face, cov = area * temperature (0 at temperature 0);
        where it is not 0, and without ``inside``, cov is as above.  The gradient is the same either way."""
        if not (0.0 <= float(temperature) <= 1.0):
            raise ValueError("temperature must be in the range [0, 1]")
        if inside is not None and tuple(inside.shape) != tuple(render_layers.shape):
            raise ValueError(f"inside must have dimensions {tuple(render_layers.shape)}, got {tuple(inside.shape)}")
        window = self._layers_window(batch_mvp_idx, render_layers, patch_min, verts.device, check_frame=False)
        if window is not None and render_layers.numel() == 0:
            return torch.empty(tuple(render_layers.shape), dtype=torch.float32, device=verts.device)
        i32, f32 = torch.int32, torch.float32
        _, verts_image = self._project(batch_mvp_idx, verts, faces, graph=True)
        with self._entered(window):
            return CoverageFunction.apply(render_layers.to(i32), verts_image.to(f32), faces.to(i32), float(temperature), inside)

    @staticmethod
    def vertex_adjacency(faces: torch.Tensor, num_verts: int):
        """The inverted index from vertices to face corners (not in the reference): faces (F,3) of any integer dtype, on the
        GPU or the CPU -> (offsets (P+1,) int32, corners (3F,) int32) on ``faces``' device, P = ``num_verts``.  A face is valid
        when its three ids lie in [0, P).  ``corners`` holds the corner numbers 3 f + k ordered by (vertex id, corner number)
        ascending, the corners of invalid faces at the end; vertex p owns ``corners[offsets[p]:offsets[p+1]]`` and
        ``offsets[P]`` is the number of valid corners.  A pure function of ``faces``, without a host read-back: build it once per
        topology and hand the pair to ``vertex_normals`` (nothing is cached behind the caller's back).  3 F must be below 2^31."""
        if faces.dim() != 2 or faces.size(1) != 3:
            raise ValueError(f"faces must have dimensions (F, 3), got {tuple(faces.shape)}")
        if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
            raise ValueError(f"faces: expected an integer dtype, got {faces.dtype}")
        P, F = int(num_verts), int(faces.size(0))
        if P < 0:
            raise ValueError("num_verts must not be negative")
        if 3 * F >= 2 ** 31:
            raise ValueError("faces: 3 * F must be below 2^31")
        with torch.no_grad():
            ids = faces.long()
            valid = ((ids >= 0) & (ids < P)).all(dim=1, keepdim=True)
            key = torch.where(valid, ids, torch.full_like(ids, P)).reshape(-1)          # (3F,): the corner's vertex, P if invalid
            skey, order = torch.sort(key, stable=True)                                   # ties keep the corner numbers ascending
            offsets = torch.searchsorted(skey, torch.arange(P + 1, device=faces.device, dtype=torch.long))
        return offsets.to(torch.int32), order.to(torch.int32)

    def vertex_normals(self, verts: torch.Tensor, faces: torch.Tensor, adjacency=None, normalize: bool = True):
        """Smooth vertex normals (not in the reference): verts (P,3), faces (F,3) -> normals (P,3) float32 = the sum of the
        vertex's face normals (p1 - p0) x (p2 - p0), unnormalised and so weighted by area, divided by its length
        (``normalize=False``: the sum itself).  A vertex without faces, or whose sum is zero or not finite, gets zeros; a face
        that names a vertex outside [0, P) contributes to none.  ``adjacency``: ``vertex_adjacency(faces, P)``, built once per
        topology; None builds it inside the call.  ``interpolate(render_layers, bary, normals, faces)`` turns the result into a
        normal image.

        Differentiable w.r.t. ``verts`` (``VertexNormalsFunction``); faces and the index are constants.  Forward and backward
        are a store pass over the faces and a gather pass over the vertices in the index's fixed order: no float atomics, and
        two calls give the same bits.  The summation order is (face id, corner) ascending per vertex."""
        i32, f32 = torch.int32, torch.float32
        if adjacency is None:
            adjacency = Renderer.vertex_adjacency(faces, verts.shape[0])
        offsets, corners = adjacency
        return VertexNormalsFunction.apply(verts.to(f32), faces.to(i32), offsets, corners, bool(normalize))

    def shading_vectors(self, batch_mvp_idx: Sequence[int], render_layers: torch.Tensor, t: torch.Tensor,
                        normals: torch.Tensor = None, patch_min: torch.Tensor = None):
        """The vectors a shader needs per slot (not in the reference): render_layers (B,H,W,L) int32 and t (B,H,W,L) as
        ``rasterize`` returns them, normals (B,H,W,L,3) of any length (``interpolate``'s output for ``vertex_normals``) or None
        -> (position, view), or with ``normals`` (position, view, normal, reflection), each (B,H,W,L,3) float32.  With (ro, rd)
        the ray of the slot's pixel, the one ``rasterize`` used (the ray tensors, or the computed ray of
        ``Renderer(analytic_rays=True)``): position = ro + t rd, the hit in world space; view = -rd, from the surface to the
        eye; normal = normals / |normals|; reflection = 2 (normal . view) normal - view, the mirror direction of the view about
        the normal, the same for n and -n: what ``texture(..., boundary_mode="cube")`` looks an environment map up by.

        A slot with a negative id or a t that is not finite is empty: zeros in every output, no gradient.  Where the normal is
        zero or not finite, normal and reflection are zero and ``normals`` gets no gradient.  Differentiable w.r.t. ``t``
        (through position) and ``normals`` (``ShadingVectorsFunction``; the normal's gradient is orthogonal to it); view is a
        constant, and nothing flows to the cameras.

        Window: with ``patch_min`` (B,2) int32, render_layers is a window's and slot (b, y, x) is frame pixel
        (x + patch_min[b,0], y + patch_min[b,1]): the crop of the full-frame result.  Checks and errors are ``coverage``'s; an
        empty window launches nothing."""
        i32, f32 = torch.int32, torch.float32
        window = self._layers_window(batch_mvp_idx, render_layers, patch_min, render_layers.device, check_frame=True)
        if window is not None and render_layers.numel() == 0:
            return tuple(torch.empty(tuple(render_layers.shape) + (3,), dtype=f32, device=render_layers.device)
                         for _ in range(2 if normals is None else 4))
        nrm = None if normals is None else normals.to(f32)
        ray_o, ray_d, ctx = self._rays(batch_mvp_idx, window)
        with ctx:
            return ShadingVectorsFunction.apply(render_layers.to(i32), t.to(f32), nrm, ray_o, ray_d)

    def _forward_with_rays(self, batch_mvp_idx, ray_o, ray_d, batch_patch_min, patch_width, patch_height, verts, faces,
                           verts_color, faces_opacity, faces_intense, background, aa_temperature):
        B, F, f32 = len(batch_mvp_idx), faces.shape[0], torch.float32
        if getattr(self, "fused_prep", False) and verts.is_cuda:
            from . import prep
            tfi = getattr(self, "tables_from_image", None)
            if _FUSED_AA_GRAD and (_TABLES_FROM_IMAGE if tfi is None else tfi):
                # the fused prep owns the AA tables end to end: they are never materialised -- the op's plan builds them per
                # face from verts_image straight into its packed records (DM2_FLAG_TABLES_FROM_IMAGE; 114 B per face less to
                # write and to read back), and the corner gradients come back per vertex, as the gradient of verts_image
                verts_ndc, verts_image = self._project(batch_mvp_idx, verts, faces, graph=True)
                ph4 = torch.empty((B, 0, 3, 2), dtype=f32, device=verts.device)
                with _C.tables_from_image(True), _C.aa_grad_to_verts(True):
                    out = RenderFunction.apply(
                        background.to(f32), batch_patch_min.to(torch.int32), patch_width, patch_height,
                        verts.to(f32), faces.to(torch.int32), verts_color.to(f32), faces_opacity.to(f32),
                        verts_ndc, verts_image, faces_intense.to(f32), aa_temperature,
                        ph4, ph4, ph4.to(torch.bool), ph4, ph4, torch.empty((B, 0, 3), dtype=f32, device=verts.device),
                        self.aa_grad_buffer_size, ray_o, ray_d)
                return _finish(out)
            (verts_ndc, verts_image, aa_v, aa_e, aa_z, aa_r, aa_n, aa_c) = prep.prepare(
                verts.to(f32), faces.to(torch.int32), self.mv[batch_mvp_idx].to(f32), self.proj[batch_mvp_idx].to(f32), self.width,
                self.height)
            # the fused prep owns both ends of aa_face_verts: the op hands its corner gradients back per VERTEX (as the
            # gradient of verts_image) and prepare_faces_backward needs no (B,F,3,2) scatter pass (DM2_FUSED_AA_GRAD=0: the
            # reference's route through dL/d(aa_face_verts))
            with _C.aa_grad_to_verts(_FUSED_AA_GRAD and verts_image.requires_grad):
                out = RenderFunction.apply(
                    background.to(f32), batch_patch_min.to(torch.int32), patch_width, patch_height,
                    verts.to(f32), faces.to(torch.int32), verts_color.to(f32), faces_opacity.to(f32),
                    verts_ndc, verts_image, faces_intense.to(f32), aa_temperature,
                    aa_v, aa_e, aa_z, aa_r, aa_n, aa_c, self.aa_grad_buffer_size, ray_o, ray_d)
            return _finish(out)
        verts_ndc, verts_image = self._project(batch_mvp_idx, verts, faces, graph=True)

        corners = verts_image[:, faces.flatten()].view(-1, 3, 2)             # (B*F,3,2)
        tri = Triangles(corners[:, 0], corners[:, 1], corners[:, 2])
        out = RenderFunction.apply(
            background.to(f32),
            batch_patch_min.to(torch.int32), patch_width, patch_height,
            verts.to(f32), faces.to(torch.int32), verts_color.to(f32), faces_opacity.to(f32),
            verts_ndc.to(f32), verts_image.to(f32), faces_intense.to(f32),
            aa_temperature,
            tri.verts.reshape(B, F, 3, 2).to(f32),
            tri.edges.reshape(B, F, 3, 2).to(f32),
            tri.edges_iszero.reshape(B, F, 3, 2).to(torch.bool),
            tri.edges_recip.reshape(B, F, 3, 2).to(f32),
            tri.edges_normal.reshape(B, F, 3, 2).to(f32),
            tri.edges_normal_c.reshape(B, F, 3).to(f32),
            self.aa_grad_buffer_size,
            ray_o, ray_d,
        )
        return _finish(out)


def _finish(out):
    """RenderFunction's (color, depth[, alpha]) -> Renderer's: NDC z in [-1,1] (background +1) -> [0,1] with background 0
    (reference :377-378)."""
    return (out[0], 1.0 - (out[1] + 1.0) / 2.0) + tuple(out[2:])


class LayeredCompositeFunction(torch.autograd.Function):
    """Differentiable front-to-back compositing of per-pixel face layers (``_C.composite_layers_cuda``).

    Inputs: render_layers (B,H,W,L) int32 (ids outside [0, F) are skipped), verts (P,3), faces (F,3) int32,
    verts_color (P,3)*, faces_opacity (F)*, faces_intense (B,F)*, verts_ndc (B,P,3)* [grad only in z], background (3),
    image_ray_o, image_ray_d (B,H,W,3) (placeholders under ``_C.analytic_rays``).  Outputs: color (B,H,W,3) and the raw
    NDC depth (B,H,W), background 1.  (* = receives a gradient.)

    Per pixel a layer blends where the pixel's ray hits its face inside the triangle (Renderer's coverage at
    aa_temperature 0), with the same colour, depth and alpha as Renderer.  No gradient reaches ``verts`` through the
    barycentrics: layers from the tet walk are piecewise constant in the points, and DMesh++ holds the points fixed on
    this path.  ``background`` gets no gradient, as in Renderer.

    Under ``_C.alpha_output(True)`` a third output: alpha (B,H,W) = 1 - final_T, with a gradient w.r.t. faces_opacity; an
    alpha left out of the loss launches the kernel of the two-output function.  Under ``_C.face_weights_output(True)`` a last
    output: face_weights (B,F), the sum of alpha * T over each face's blends, non-differentiable.
    """

    @staticmethod
    def forward(ctx, render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background,
                image_ray_o, image_ray_d):
        (ctx.alpha,) = _hold_channels(ctx, _C.analytic_rays, _C.window, read=(_C.alpha_output,))
        if ctx.alpha:
            ctx.set_materialize_grads(False)
        out = _C.composite_layers_cuda(
            render_layers, verts.detach(), faces, verts_color.detach(), faces_opacity.detach(), faces_intense.detach(),
            verts_ndc.detach(), background, image_ray_o, image_ray_d)
        color, depth, final_T, n_contrib = out[:4]
        ctx.save_for_backward(render_layers, verts.detach(), faces, verts_color.detach(), faces_opacity.detach(),
                              faces_intense.detach(), verts_ndc.detach(), background, image_ray_o, image_ray_d, n_contrib)
        res = (color, depth, 1.0 - final_T) if ctx.alpha else (color, depth)     # (alpha bit-equal to the kernel's 1.f - T)
        if len(out) > 4:                               # face_weights_output: non-differentiable
            ctx.mark_non_differentiable(out[4])
            res += (out[4],)
        return res

    @staticmethod
    def backward(ctx, grad_color, grad_depth, *grad_rest):
        grad_alpha = grad_rest[0] if ctx.alpha else None      # (then face_weights', ignored)
        (render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background, ray_o, ray_d,
         n_contrib) = ctx.saved_tensors
        if ctx.alpha:                                  # (grads not materialised)
            grad_color, grad_depth = _image_grads(grad_color, grad_depth, n_contrib.shape, n_contrib.device)
        with _held_channels(ctx):
            extra = {} if grad_alpha is None else {"dL_dout_alpha": grad_alpha}
            dcolor, dopacity, dndc, dintense = _C.composite_layers_backward_cuda(
                render_layers, verts, faces, verts_color, faces_opacity, faces_intense, verts_ndc, background, ray_o, ray_d,
                n_contrib, grad_color, grad_depth, **extra)
        return None, None, None, dcolor, dopacity, dintense, dndc, None, None, None


def _rasterize_forward(ctx, overlap, verts, faces, faces_existence, verts_ndc, verts_image, image_ray_o, image_ray_d, width, height,
                       num_layers):
    """The forward of RasterizeFunction and RasterizeOverlapFunction (``overlap``: one more output, inside)."""
    _hold_channels(ctx, _C.analytic_rays, _C.window)
    ctx.set_materialize_grads(False)            # bary / t left out of the loss arrive as None
    ctx.mode = {"overlap": True} if overlap else {}     # (the keyword only in overlap mode: otherwise the very call it was)
    out = _C.rasterize_layers_cuda(width, height, verts.detach(), faces, faces_existence, verts_ndc.detach(), verts_image.detach(),
                                   image_ray_o, image_ray_d, num_layers, **ctx.mode)
    layers, cnt = out[:2]
    ctx.mark_non_differentiable(layers, cnt, *out[4:])
    ctx.save_for_backward(layers, verts.detach(), faces, image_ray_o, image_ray_d)
    return out


def _rasterize_backward(ctx, grad_bary, grad_t):
    if (grad_bary is None and grad_t is None) or not ctx.needs_input_grad[0]:
        return (None,) * 10
    layers, verts, faces, ray_o, ray_d = ctx.saved_tensors
    with _held_channels(ctx):
        dverts = _C.rasterize_layers_backward_cuda(layers, verts, faces, ray_o, ray_d, grad_bary, grad_t, **ctx.mode)
    return (dverts,) + (None,) * 9


class RasterizeFunction(torch.autograd.Function):
    """The first L faces each pixel's ray hits (``_C.rasterize_layers_cuda``), differentiable in bary and t w.r.t. verts.

    Inputs: verts (P,3)*, faces (F,3) int32, faces_existence (F) int32 or None, verts_ndc (B,P,3) and verts_image (B,P,2) (the
    plan's bins and depth cull: no gradient), image_ray_o, image_ray_d (B,H,W,3) (placeholders under ``_C.analytic_rays``),
    width, height, num_layers.  Outputs: render_layers (B,H,W,L) int32 and render_layers_cnt (B,H,W) int32 (not
    differentiable), bary (B,H,W,L,3), t (B,H,W,L).  (* = receives a gradient.)

    A listed hit sends (g1 - g0) du/dp + (g2 - g0) dv/dp + g_t dt/dp to its three vertices; empty slots send nothing.  When
    neither bary nor t reaches the loss no backward kernel runs.
    """

    @staticmethod
    def forward(ctx, *inputs):
        return _rasterize_forward(ctx, False, *inputs)

    @staticmethod
    def backward(ctx, grad_layers, grad_cnt, grad_bary, grad_t):
        return _rasterize_backward(ctx, grad_bary, grad_t)


class RasterizeOverlapFunction(torch.autograd.Function):
    """``Renderer.rasterize(overlap=True)``: the first L faces that overlap each pixel's square and whose plane the ray meets in
    front (``_C.rasterize_layers_cuda(..., overlap=True)``), differentiable in bary and t w.r.t. verts.

    Inputs: RasterizeFunction's.  Outputs: render_layers, render_layers_cnt, bary (B,H,W,L,3) = the clamped barycentrics, t
    (B,H,W,L), inside (B,H,W,L) bool (not differentiable, like the ids).  The backward recomputes each slot's clamp code and
    chains dL/dbary through ``clamp_bary_uv_grad`` and dL/dt through the hit's t (inside) or the projection formula (elsewhere).
    """

    @staticmethod
    def forward(ctx, *inputs):
        return _rasterize_forward(ctx, True, *inputs)

    @staticmethod
    def backward(ctx, grad_layers, grad_cnt, grad_bary, grad_t, grad_inside):
        return _rasterize_backward(ctx, grad_bary, grad_t)


class InterpolateFunction(torch.autograd.Function):
    """out = (bary0 attr[v0] + bary1 attr[v1]) + bary2 attr[v2] per slot of render_layers (``_C.interpolate_cuda``).

    Inputs: render_layers (B,H,W,L) int32, bary (B,H,W,L,3)*, attr (N,C)* or (B,N,C)*, attr_faces (F,3) int32.  Output: out
    (B,H,W,L,C).  (* = receives a gradient.)  A filled slot sends bary_k g to row v_k of attr and attr[v_k] . g to bary_k;
    empty slots send nothing and get zero.  Only the gradients ``needs_input_grad`` asks for are computed: no attr scatter
    when only bary requires grad, and the reverse.
    """

    @staticmethod
    def forward(ctx, render_layers, bary, attr, attr_faces):
        out = _C.interpolate_cuda(render_layers, bary.detach(), attr.detach(), attr_faces)
        ctx.save_for_backward(render_layers, bary.detach(), attr.detach(), attr_faces)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        need_bary, need_attr = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if grad_out is None or not (need_bary or need_attr):
            return None, None, None, None
        render_layers, bary, attr, attr_faces = ctx.saved_tensors
        dattr, dbary = _C.interpolate_backward_cuda(render_layers, bary, attr, attr_faces, grad_out, need_attr, need_bary)
        return None, dbary, dattr, None


class _LookupFunction(torch.autograd.Function):
    """The body of the per-slot lookup Functions.  Their inputs are ``tensors`` leading tensors (detached and saved), render_layers
    (saved, may be None) and the modes; a subclass names its ``_C`` entry pair (``<entry>_cuda``, ``<entry>_backward_cuda``, looked
    up on ``_C`` at call time) and, in ``grads``, the input positions that receive a gradient, in the order in which the backward
    entry takes their ``need_*`` flags and returns their gradients."""
    entry, tensors, grads = None, 0, ()

    @classmethod
    def forward(cls, ctx, *inputs):
        detached = [t.detach() for t in inputs[:cls.tensors]]
        ctx.modes = inputs[cls.tensors + 1:]
        out = getattr(_C, cls.entry + "_cuda")(*detached, *inputs[cls.tensors:])
        _save_optional(ctx, *detached, inputs[cls.tensors])
        return out

    @classmethod
    def backward(cls, ctx, grad_out):
        needs = [ctx.needs_input_grad[i] for i in cls.grads]
        grads = [None] * (cls.tensors + 1 + len(ctx.modes))
        if grad_out is not None and any(needs):
            got = getattr(_C, cls.entry + "_backward_cuda")(*_saved_optional(ctx), *ctx.modes, grad_out, *needs)
            for i, g in zip(cls.grads, got):
                grads[i] = g
        return tuple(grads)


class TextureFunction(_LookupFunction):
    """out = the texture at each slot's uv (``_C.texture_cuda``): bilinear a + fy (b - a) over the four texels round
    (u Wt - 0.5, v Ht - 0.5), or the nearest texel; wrap or clamp addressing.

    Inputs: uv (B,H,W,L,2)*, tex (Ht,Wt,C)* or (B,Ht,Wt,C)*, render_layers (B,H,W,L) int32 or None, filter_mode, boundary_mode.
    Output: out (B,H,W,L,C).  (* = receives a gradient.)  A non-empty slot sends w_pq g to its four texels and the texture's
    finite differences . g to (u, v) (zeros for nearest); empty slots send nothing and get zero.  Only the gradients
    ``needs_input_grad`` asks for are computed: no texel scatter when only uv requires grad, and the reverse.
    """

    entry, tensors, grads = "texture", 2, (1, 0)


class TextureCubeFunction(_LookupFunction):
    """out = the cube map in each slot's direction (``_C.texture_cube_cuda``): the major axis picks the face, bilinear over four
    taps that continue onto the adjacent face across an edge (three renormalised taps at a cube corner), or the nearest texel.

    Inputs: dirs (B,H,W,L,3)*, tex (6,N,N,C)* or (B,6,N,N,C)*, render_layers (B,H,W,L) int32 or None, filter_mode.
    Output: out (B,H,W,L,C).  (* = receives a gradient.)  A non-empty slot sends w_k g to its texels and, through the face
    coordinates sc / ma and tc / ma, a gradient orthogonal to the direction (zeros for nearest); empty slots send nothing and
    get zero.  Only the gradients ``needs_input_grad`` asks for are computed.
    """

    entry, tensors, grads = "texture_cube", 2, (1, 0)


class TextureVolumeFunction(_LookupFunction):
    """out = the voxel grid at each slot's position (``_C.texture_volume_cuda``): trilinear a0 + fz (a1 - a0) over the bilinear
    blends of the two planes round (x N - 0.5, y N - 0.5, z N - 0.5), or the nearest voxel; clamp or wrap addressing.

    Inputs: xyz (B,H,W,L,3)*, grid (N,N,N,C)* or (B,N,N,N,C)*, render_layers (B,H,W,L) int32 or None, filter_mode,
    boundary_mode.  Output: out (B,H,W,L,C).  (* = receives a gradient.)  A non-empty slot sends w_pqr g to its eight voxels and
    the grid's finite differences . g to (x, y, z) (zeros for nearest); empty slots send nothing and get zero.  Only the
    gradients ``needs_input_grad`` asks for are computed: no voxel scatter when only xyz requires grad, and the reverse.
    """

    entry, tensors, grads = "texture_volume", 2, (1, 0)


class HashGridFunction(_LookupFunction):
    """out = the hash grid's levels at each slot's position (``_C.hash_grid_cuda``): per level ``TextureVolumeFunction``'s lookup
    of a virtual R_l^3 grid whose voxels live in rows of table[l], by position while the level fits and by hash after that.

    Inputs: xyz (B,H,W,L,3)*, table (NL,T,F)*, render_layers (B,H,W,L) int32 or None, base_resolution, growth, filter_mode,
    boundary_mode.  Output: out (B,H,W,L,NL*F).  (* = receives a gradient.)  A non-empty slot sends w_pqr g to its eight rows of
    every level and the levels' finite differences . g, scaled by R_l, to (x, y, z) (zeros for nearest); empty slots send nothing
    and get zero.  Only the gradients ``needs_input_grad`` asks for are computed.
    """

    entry, tensors, grads = "hash_grid", 2, (1, 0)


class BaryDerivativesFunction(torch.autograd.Function):
    """(dbary_dx, dbary_dy) = the derivatives of each listed slot's barycentrics with respect to the pixel position
    (``_C.bary_derivatives_cuda``).

    Inputs: render_layers (B,H,W,L) int32, verts (P,3), faces (F,3) int32, ray_cam (B,32) = inv(mv), inv(proj) per view.  Outputs:
    two (B,H,W,L,3) tensors, both marked non-differentiable: the footprint is a constant of the pipeline (nothing flows to
    ``verts`` through it, as nothing flows through which faces are listed)."""

    @staticmethod
    def forward(ctx, render_layers, verts, faces, ray_cam):
        dx, dy = _C.bary_derivatives_cuda(render_layers, verts.detach(), faces, ray_cam.detach())
        ctx.mark_non_differentiable(dx, dy)
        return dx, dy

    @staticmethod
    def backward(ctx, grad_dx, grad_dy):
        return None, None, None, None


class MipmapFunction(torch.autograd.Function):
    """mip = the chain of 2 x 2 means of a texture (``_C.texture_mipmaps_cuda``).

    Inputs: tex (Ht,Wt,C)* or (B,Ht,Wt,C)*, max_mip_level (int or None).  Output: mip (T,C) or (B,T,C), levels 1 .. nlev-1.
    (* = receives a gradient.)  Every texel of dL/dtex is the sum over the levels of 0.25^k times the gradient of the level-k
    texel above it: a gather, deterministic."""

    @staticmethod
    def forward(ctx, tex, max_mip_level):
        ctx.max_mip_level = max_mip_level
        ctx.save_for_backward(tex.detach())
        return _C.texture_mipmaps_cuda(tex.detach(), max_mip_level)

    @staticmethod
    def backward(ctx, grad_mip):
        if grad_mip is None or not ctx.needs_input_grad[0]:
            return None, None
        (tex,) = ctx.saved_tensors
        return _C.texture_mipmaps_backward_cuda(tex, ctx.max_mip_level, grad_mip), None


class CubePrefilterFunction(torch.autograd.Function):
    """out = the GGX prefilter of a cube's mip chain, un-normalised (``_C.cube_prefilter_cuda``): level k convolved with the
    lobe of roughness k / (nlev - 1), out[o] = sum_s K(o,s) Om_s chain[s].

    Inputs: chain (6,T,C)* or (B,6,T,C)*, N, max_mip_level (int or None).  Output: the same shape.  (* = receives a gradient.)
    The filter is linear and K symmetric: dL/dchain[s] = Om_s sum_o K(o,s) g[o] (``_C.cube_prefilter_transpose_cuda``), a
    gather like the forward, deterministic."""

    @staticmethod
    def forward(ctx, chain, N, max_mip_level):
        ctx.sizes = (N, max_mip_level)
        return _C.cube_prefilter_cuda(chain.detach(), N, max_mip_level)

    @staticmethod
    def backward(ctx, grad_out):
        if grad_out is None or not ctx.needs_input_grad[0]:
            return None, None, None
        return _C.cube_prefilter_transpose_cuda(grad_out, *ctx.sizes), None, None


class TextureMipFunction(_LookupFunction):
    """out = the trilinear sample of a texture and its mip chain at each slot's uv (``_C.texture_mip_cuda``): the bilinear
    samples c_j, c_{j+1} of the two levels round the slot's level of detail, c_j + f (c_{j+1} - c_j); one level at or below
    level 0 and beyond the last.

    Inputs: uv (B,H,W,L,2)*, uv_da (B,H,W,L,4), tex (Ht,Wt,C)* or (B,Ht,Wt,C)*, mip (T,C)* or (B,T,C)*, render_layers (B,H,W,L)
    int32 or None, boundary_mode, max_mip_level.  Output: out (B,H,W,L,C).  (* = receives a gradient.)  A non-empty slot sends
    (1 - f) w_pq g and f w_pq g to the texels of its two levels (level 0's in tex, the others in mip) and the blend of the two
    levels' finite differences . g to (u, v); uv_da gets none: the level of detail is a constant of the op.  Only the gradients
    ``needs_input_grad`` asks for are computed."""

    entry, tensors, grads = "texture_mip", 4, (2, 3, 0)


class TextureCubeMipFunction(_LookupFunction):
    """out = the cube map and its mip chain in each slot's direction at the slot's level of detail
    (``_C.texture_cube_mip_cuda``): c_j + f (c_{j+1} - c_j) of the cube samples of the two levels round the level; one level
    at or below level 0 and at or beyond the last.

    Inputs: dirs (B,H,W,L,3)*, mip_level (B,H,W,L)*, tex (6,N,N,C)* or (B,6,N,N,C)*, mip (6,T,C)* or (B,6,T,C)*, render_layers
    (B,H,W,L) int32 or None, max_mip_level.  Output: out (B,H,W,L,C).  (* = receives a gradient.)  A non-empty slot sends
    (1 - f) w g and f w g to the texels of its two levels (level 0's in tex, the others in mip), the blend of the two levels'
    direction gradients to dirs, and g . (c_{j+1} - c_j) to its level (0 where the level is clamped).  Only the gradients
    ``needs_input_grad`` asks for are computed."""

    entry, tensors, grads = "texture_cube_mip", 4, (2, 3, 0, 1)


class CompositeFunction(torch.autograd.Function):
    """out, acc = the front-to-back blend of per-slot values (``_C.composite_cuda``): O += values (a T), T *= 1 - a over the
    non-empty slots until T < 1e-4; out = O + T background, acc = 1 - T.

    Inputs: values (B,H,W,L,C)*, alpha (B,H,W,L)* per slot or (F,)* per face, render_layers (B,H,W,L) int32 or None, background
    (C,) or None.  Outputs: out (B,H,W,C), acc (B,H,W).  (* = receives a gradient.)  A blended slot gets (a T) g for its values
    and T (S - R) for its alpha (the back pass of include/dm2_hip.h, no division); empty slots and slots behind the stop get
    zeros.  Output gradients are not materialised: an output left out of the loss costs nothing, and with both left out no
    kernel runs.  Only the gradients ``needs_input_grad`` asks for are computed.
    """

    @staticmethod
    def forward(ctx, values, alpha, render_layers, background):
        ctx.set_materialize_grads(False)
        out, acc, _, n_contrib = _C.composite_cuda(values.detach(), alpha.detach(), render_layers, background)
        _save_optional(ctx, values.detach(), alpha.detach(), n_contrib, render_layers, background)
        return out, acc

    @staticmethod
    def backward(ctx, grad_out, grad_acc):
        need_values, need_alpha = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (grad_out is None and grad_acc is None) or not (need_values or need_alpha):
            return None, None, None, None
        values, alpha, n_contrib, render_layers, background = _saved_optional(ctx)
        dvalues, dalpha = _C.composite_backward_cuda(values, alpha, render_layers, background, n_contrib, grad_out, grad_acc,
                                                     need_values, need_alpha)
        return dvalues, dalpha, None, None


class CoverageFunction(torch.autograd.Function):
    """cov = the analytic overlap of each listed face with its pixel, mixed with the temperature (``_C.coverage_cuda``):
    (1 - temperature) + area * temperature; 0 in an empty slot, where the clipper errs and where the area is 0.

    Inputs: render_layers (B,H,W,L) int32, verts_image (B,P,2)*, faces (F,3) int32, temperature, inside (B,H,W,L) bool or integer
    or None (a slot where it is 0 mixes as area * temperature; the gradient does not need it).  Output: cov (B,H,W,L).
    (* = receives a gradient.)  A partially covered slot sends g temperature d(area)/d(corner) to the image coordinates of its
    face's three vertices; nothing flows through which faces are listed.  The output gradient is not materialised: with cov
    left out of the loss, or at temperature 0, no kernel runs.
    """

    @staticmethod
    def forward(ctx, render_layers, verts_image, faces, temperature, inside=None):
        ctx.set_materialize_grads(False)
        _hold_channels(ctx, _C.window)              # (origins, frame size) of a window call: kept for the backward
        cov = _C.coverage_cuda(render_layers, verts_image.detach(), faces, temperature, inside)
        ctx.temperature = float(temperature)
        ctx.save_for_backward(render_layers, verts_image.detach(), faces)
        return cov

    @staticmethod
    def backward(ctx, grad_cov):
        if grad_cov is None or ctx.temperature == 0.0 or not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        render_layers, verts_image, faces = ctx.saved_tensors
        with _held_channels(ctx):
            return None, _C.coverage_backward_cuda(render_layers, verts_image, faces, ctx.temperature, grad_cov), None, None, None


class VertexNormalsFunction(torch.autograd.Function):
    """normals = the area-weighted sum of each vertex's face normals, normalised or not (``_C.vertex_normals_cuda``).

    Inputs: verts (P,3)*, faces (F,3) int32, offsets (P+1,) int32, corners (3F,) int32 (``Renderer.vertex_adjacency``),
    normalize.  Output: normals (P,3).  (* = receives a gradient.)  The backward is a store pass over the faces and a gather
    pass over the vertices through the same index: no float atomics, the same bits on every call.  The output gradient is not
    materialised: with the normals left out of the loss, or ``verts`` not requiring a gradient, no kernel runs.
    """

    @staticmethod
    def forward(ctx, verts, faces, offsets, corners, normalize):
        ctx.set_materialize_grads(False)
        normals, lens = _C.vertex_normals_cuda(verts.detach(), faces, offsets, corners, normalize)
        ctx.normalize = bool(normalize)
        ctx.save_for_backward(verts.detach(), faces, offsets, corners, normals, lens)
        return normals

    @staticmethod
    def backward(ctx, grad_normals):
        if grad_normals is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        verts, faces, offsets, corners, normals, lens = ctx.saved_tensors
        return _C.vertex_normals_backward_cuda(verts, faces, offsets, corners, ctx.normalize, normals, lens, grad_normals), None, None, \
            None, None


class ShadingVectorsFunction(torch.autograd.Function):
    """(position, view[, normal, reflection]) per slot from rasterize's t, the pixel's ray and interpolate's normal
    (``_C.shading_vectors_cuda``): position = ro + t rd, view = -rd, normal = n / |n|, reflection = 2 (normal . view) normal - view.

    Inputs: render_layers (B,H,W,L) int32, t (B,H,W,L)*, normals (B,H,W,L,3)* or None, image_ray_o, image_ray_d (B,H,W,3)
    (placeholders under ``_C.analytic_rays``; under ``_C.window`` the window's cut).  Outputs: two or four (B,H,W,L,3) tensors.
    (* = receives a gradient.)  ``view`` is marked non-differentiable and nothing flows to the rays.  Output gradients are not
    materialised: an output left out of the loss costs nothing, and only the gradients ``needs_input_grad`` asks for are
    computed; where none is, no kernel runs.
    """

    @staticmethod
    def forward(ctx, render_layers, t, normals, image_ray_o, image_ray_d):
        ctx.set_materialize_grads(False)
        _hold_channels(ctx, _C.analytic_rays, _C.window)
        ctx.has_normals = normals is not None
        outs = _C.shading_vectors_cuda(render_layers, t.detach(), None if normals is None else normals.detach(), image_ray_o,
                                       image_ray_d)
        _save_optional(ctx, render_layers, t.detach(), image_ray_o, image_ray_d, None if normals is None else normals.detach())
        ctx.mark_non_differentiable(outs[1])
        return outs

    @staticmethod
    def backward(ctx, g_position, g_view, g_normal=None, g_reflection=None):
        need_t = ctx.needs_input_grad[1] and g_position is not None
        need_n = ctx.has_normals and ctx.needs_input_grad[2] and (g_normal is not None or g_reflection is not None)
        if not (need_t or need_n):
            return None, None, None, None, None
        render_layers, t, ray_o, ray_d, normals = _saved_optional(ctx)
        with _held_channels(ctx):
            dt, dn = _C.shading_vectors_backward_cuda(render_layers, t, normals, ray_o, ray_d, g_position, g_normal, g_reflection,
                                                      need_t, need_n)
        return None, dt, dn, None, None


class LayeredRenderer(Renderer):
    """Reference ``LayeredRenderer`` (__init__.py:388-451): non-differentiable per-pixel face layers (``generate``).

    Not in the reference: ``render`` composites such layers into an image, differentiably.  (The reference skips
    ``nn.Module.__init__``; here the module is initialised properly, which changes nothing observable.)
    """

    def __init__(self, mv, proj, width, height, device, fused_prep=None, analytic_rays=False):
        torch.nn.Module.__init__(self)
        self.analytic_rays = bool(analytic_rays)
        self._setup(mv, proj, width, height, device)
        self.fused_prep = _FUSED_PREP_DEFAULT if fused_prep is None else bool(fused_prep)

    def generate(self, batch_mvp_idx: Sequence[int], verts: torch.Tensor, faces: torch.Tensor,
                 tets: torch.Tensor, face_tets: torch.Tensor, tet_faces: torch.Tensor,
                 faces_existence: torch.Tensor, num_layers: int, patch_min: torch.Tensor = None, patch_width: int = None,
                 patch_height: int = None):
        """-> render_layers (B,H,W,L) int32 face ids (-1 = empty), render_layers_cnt (B,H,W) int32.

        Not in the reference: ``patch_min`` (B,2) int32 (x, y) per selected view with ``patch_width``, ``patch_height``
        generates the layers of that window of each view only (H, W = patch_height, patch_width): window pixel (x, y) is frame
        pixel (x + patch_min[b,0], y + patch_min[b,1]) with that pixel's ray, the first-hit pass's 16x16 tiles anchored at the
        window's origin -- ``Renderer.rasterize``'s window rules and errors."""
        window = self._sized_window(batch_mvp_idx, patch_min, patch_width, patch_height, verts.device)
        pw, ph = (self.width, self.height) if window is None else (window.width, window.height)
        i32, f32 = torch.int32, torch.float32
        B, dev = len(batch_mvp_idx), verts.device
        if window is not None and window.empty:
            return torch.empty((B, ph, pw, int(num_layers)), dtype=i32, device=dev), torch.empty((B, ph, pw), dtype=i32, device=dev)
        verts_ndc, verts_image = self._project(batch_mvp_idx, verts, faces, graph=False)
        ray_o, ray_d, ctx = self._rays(batch_mvp_idx, window)
        with ctx:
            return _C.generate_render_layers_cuda(
                pw, ph, verts.to(f32), faces.to(i32), tets.to(i32), face_tets.to(i32), tet_faces.to(i32), faces_existence.to(i32),
                verts_ndc.to(f32), verts_image.to(f32), ray_o, ray_d, int(num_layers))

    def render(self, batch_mvp_idx: Sequence[int], render_layers: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor,
               verts_color: torch.Tensor, faces_opacity: torch.Tensor, faces_intense: torch.Tensor, background: torch.Tensor,
               return_alpha: bool = False, return_face_weights: bool = False, patch_min: torch.Tensor = None):
        """Composite per-pixel face layers front to back -> color (B,H,W,3), depth (B,H,W) in [0,1] (0 = background); with
        ``return_alpha=True`` also alpha (B,H,W) = 1 - T, differentiable w.r.t. faces_opacity; with
        ``return_face_weights=True`` last face_weights (B,F), the sum of faces_opacity * T over each face's blends (a face
        listed twice in a pixel counts twice), not differentiable.

        render_layers (B,H,W,L) int32 over the full frame, e.g. from ``generate`` (-1 and any id outside [0, F) is skipped,
        holes included); faces_intense (B,F) of the selected views.  A layer blends where the pixel's ray hits its face
        inside the triangle, with Renderer's colour, depth and alpha at aa_temperature 0 (LayeredCompositeFunction).
        Gradients reach verts_color, faces_opacity, faces_intense, and verts through the projected depth only (as in
        Renderer); none goes through the barycentrics, in which the layers are piecewise constant.  Cameras that require
        grad get theirs the same way, through verts_ndc z.

        Window: with ``patch_min`` (B,2) int32 (x, y) per selected view, render_layers is a window's (``generate`` /
        ``rasterize`` with the same ``patch_min``; its own H, W are the window's size), each pixel takes the ray of frame pixel
        (x + patch_min[b,0], y + patch_min[b,1]), and the images are the window's: the crop of the full-frame result.  The
        window must lie inside the frame (``select_rays``' assertions; ValueError for a negative origin); an empty window
        returns empty images and launches nothing.
        """
        window = self._layers_window(batch_mvp_idx, render_layers, patch_min, verts.device, check_frame=False)
        i32, f32 = torch.int32, torch.float32
        if window is not None and window.empty:
            B, ph, pw, dev = len(batch_mvp_idx), window.height, window.width, verts.device
            out = (torch.empty((B, ph, pw, 3), dtype=f32, device=dev), torch.empty((B, ph, pw), dtype=f32, device=dev))
            if return_alpha:
                out += (torch.empty((B, ph, pw), dtype=f32, device=dev),)
            if return_face_weights:
                out += (torch.zeros((B, faces.shape[0]), dtype=f32, device=dev),)
            return out
        verts_ndc, _ = self._project(batch_mvp_idx, verts, faces, graph=True)
        ray_o, ray_d, ctx = self._rays(batch_mvp_idx, window)
        with ctx, _C.alpha_output(return_alpha), _C.face_weights_output(return_face_weights):
            out = LayeredCompositeFunction.apply(render_layers.to(i32), verts.to(f32), faces.to(i32), verts_color.to(f32),
                                                 faces_opacity.to(f32), faces_intense.to(f32), verts_ndc.to(f32), background.to(f32),
                                                 ray_o, ray_d)
        # NDC z in [-1,1] (background +1) -> [0,1] with background 0, as Renderer.forward
        return _finish(out)
