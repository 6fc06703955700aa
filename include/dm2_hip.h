/* dm2_hip.h -- C ABI of libdm2_hip.so, the MI355X (gfx950) rasterizer hot path.
 *
 * Drop-in boundary: these entry points are what the reference's pybind module
 * `dmesh2_renderer._C` (ext.cpp:5-9) binds, with torch types replaced by raw
 * device pointers + sizes.  A binding (pybind/ctypes/cffi) allocates outputs
 * and scratch with its own allocator, then calls:
 *
 *   render_forward_cuda        (render.h:12-45,  render.cu:28-195)
 *       -> dm2_forward_plan() + dm2_forward_run()
 *   render_backward_cuda       (render.h:47-94,  render.cu:198-373)
 *       -> dm2_backward()
 *   generate_render_layers_cuda(render.h:101-119, render.cu:378-476)
 *       -> dm2_layers_plan() + dm2_layers_run()
 *
 * One entry point per operation: what an operation can do in addition (a render
 * window, one more output, one more upstream gradient) is a nullable pointer of
 * its one symbol, and NULL there costs nothing -- the kernels without that work run.
 *
 * The plan/run split replaces the reference's resize-callback lambdas
 * (render.cu:20-26, renderer.cu:174-183): the number of (tile,face) pairs is
 * data dependent, so `plan` bins the faces, returns the pair count (and the
 * length of the longest tile list, which picks `run`'s sorting method), and
 * the caller sizes the binning scratch before `run`.
 *
 * All pointers are DEVICE pointers to contiguous row-major arrays unless noted.
 * All functions enqueue on `stream` (a hipStream_t passed as void*; NULL = the
 * null stream); only the plan functions wait for the GPU: for two words their last kernel stores
 * into mapped host memory (polled; a copy + event takes over where such stores are not seen in time).
 * Return value: 0 on success, non-zero on error with a message available from
 * dm2_last_error() (thread local).  The library keeps no global state besides
 * a per-thread pinned staging word.
 */
#ifndef DM2_HIP_H
#define DM2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM2_ABI_VERSION 8
#define DM2_TILE 16 /* config.h:4-5 BLOCK_X = BLOCK_Y = 16 */

/* Inputs of Renderer's op, same meaning and order as render.h:13-45. */
typedef struct dm2_render_desc {
    int32_t B, P, F;              /* views, vertices, faces */
    int32_t W, H;                 /* patch_width, patch_height */
    int32_t K;                    /* len_oarea_buffer (forced to 0 when aa_temperature == 0, render.cu:141-142) */
    float aa_temperature;         /* in [0,1] */
    int32_t flags;                /* DM2_FLAG_* */
    int32_t full_W, full_H;       /* DM2_FLAG_ANALYTIC_RAYS: size of the image the cameras' rays belong to (Renderer.width/height) */
    const float* background;      /* (3) */
    const int32_t* patch_min;     /* (B,2) */
    const float* verts;           /* (P,3) */
    const int32_t* faces;         /* (F,3) */
    const float* verts_color;     /* (P,3) */
    const float* faces_opacity;   /* (F) */
    const float* verts_ndc;       /* (B,P,3) */
    const float* verts_image;     /* (B,P,2) */
    const float* faces_intense;   /* (B,F) */
    const float* aa_face_verts;             /* (B,F,3,2) */
    const float* aa_face_edges;             /* (B,F,3,2) */
    const uint8_t* aa_face_edges_iszero;    /* (B,F,3,2) bool */
    const float* aa_face_edges_recip;       /* (B,F,3,2) */
    const float* aa_face_edges_normal;      /* (B,F,3,2) */
    const float* aa_face_edges_normal_c;    /* (B,F,3) */
    const float* image_ray_o;     /* (B,H,W,3); may be NULL with DM2_FLAG_ANALYTIC_RAYS */
    const float* image_ray_d;     /* (B,H,W,3); may be NULL with DM2_FLAG_ANALYTIC_RAYS */
    const float* ray_cam;         /* DM2_FLAG_ANALYTIC_RAYS: (B,32) = inv(mv) then inv(proj) of each view, row-major 4x4 each */
} dm2_render_desc;

/* flags */
#define DM2_FLAG_CORRECTED_DV 1  /* backward: use the true d(bary v)/d(verts) instead of the
                                    reference's as-written d(t)/d(verts) (auxiliary.h:272-280) */

#define DM2_FLAG_LEGACY_KERNELS 2 /* composite kernels: per-pixel list walk (reference-shaped work distribution)
                                    instead of the dense (pixel,face)-pair kernels; tile lists: one global radix sort
                                    instead of per-tile sorts; same results, kept for A/B */

#define DM2_FLAG_NO_BACKWARD 4    /* forward only: no backward will follow (inference, torch.no_grad()): the forward skips the per-entry
                                    blend masks it otherwise leaves for dm2_backward (32 B per list entry).  A backward called
                                    anyway still works: it takes the mask-free per-pixel walk. */

#define DM2_FLAG_ANALYTIC_RAYS 8  /* the primary rays are not read from image_ray_o / image_ray_d but computed per pixel from ray_cam
                                    in the operation order of the reference's Renderer._init_rays (__init__.py:198-237): pixel
                                    centre -> NDC (x, y, -1, 1) @ inv(proj)^T @ inv(mv)^T, NO perspective divide, direction
                                    normalised with + 1e-6 on the length.  Saves the two (B,H,W,3) tensors (49.8 MB per camera at
                                    1080p) and 24 B per pixel of reads in either pass. */

#define DM2_FLAG_AA_GRAD_TO_VERTS 16 /* dm2_backward: the sixth output is not dL/d(aa_face_verts) (B,F,3,2) but that gradient already
                                    scattered to the vertices it belongs to: a (B,P,2) array, zero-filled by the caller, that
                                    receives dL/d(aa corner) at [b, vertex of that corner] (the CCW reorder of pyrenderer.py:8,521-529
                                    undone: the forward's packed record remembers it).  What torch autograd does with
                                    dL/d(aa_face_verts) in the reference's host prep, without the (B,F,3,2) round trip: for a caller
                                    that owns the host prep as well (dmesh2_renderer_amd/prep.py).  The flag must be set in the
                                    forward call of the same frame too: that is when the record notes the reorder. */

#define DM2_FLAG_TABLES_FROM_IMAGE 32 /* dm2_forward_plan / dm2_forward: the six aa_* tables are not read (their pointers may be NULL): the plan builds them
                                    per (view, face) from verts_image[faces] in registers -- CCW reorder, edges, |e| < 1e-3 flags,
                                    reciprocals, inward normals and their offsets, exactly as pyrenderer.py:6-30 / dm2_prepare_faces
                                    compute them -- straight into its packed face records.  For a caller that owns the host prep
                                    (SURVEY.md 8(f) rank 1): 114 B per face less to write and 114 to read.  The backward's dL/d(aa
                                    corners) then only exists per vertex: combine with DM2_FLAG_AA_GRAD_TO_VERTS. */

#define DM2_FLAG_NO_PAIR_POOL 64   /* dm2_forward_run / dm2_forward: leave blend masks only (DM2_FWD_MASKS), whatever room the binning scratch has behind
                                    its fixed part: for a caller that finds the plan's pair_bound too large for its memory budget */

/* Scratch kinds for dm2_scratch_bytes (state.h:18-61). */
enum {
    DM2_SCRATCH_FACE = 0,     /* count = B*F, aux = 2 * (B*tiles) + 1 for Renderer (holds the packed face records,
                                 256 B per (view, face), that forward AND backward read), 2 * (B*tiles) for
                                 LayeredRenderer; tiles = ceil(W/16) * ceil(H/16) */
    DM2_SCRATCH_IMAGE = 1,    /* count = B*H*W, aux = B*tiles      */
    DM2_SCRATCH_BINNING = 2,  /* count = num_rendered, aux = B*tiles */
    DM2_SCRATCH_LAYER_IMAGE = 3, /* count = B*H*W, aux = B*tiles (dm2_layers_run; dm2_rasterize_run uses its tile ranges) */
    DM2_SCRATCH_LAYER_TETS = 4,  /* count = T (tets): packed per-tet records of the layer walk, 256 B each */
    DM2_SCRATCH_PAIR_POOL = 5,   /* count = pair_bound of the plan: bytes to APPEND to the binning scratch (behind its
                                    DM2_SCRATCH_BINNING bytes for the same num_rendered) for the forward's pair pool: 4 B per
                                    (pixel, face) pair, the coverage the backward would otherwise clip for again */
    DM2_SCRATCH_TIE_QUEUE = 6    /* count = pairs the binning scratch's pool part holds (appended bytes / 4): scratch of ONE
                                    dm2_backward call, 16 B per pair, written only for the pairs the exact clipper has to redo */
};

/* What a forward left for its backward: returned by dm2_forward / dm2_forward_run, to be handed to dm2_backward. */
#define DM2_FWD_UNKNOWN 0  /* dm2_backward decides on the device: every candidate kernel is launched, all but one return at once */
#define DM2_FWD_NONE 1     /* nothing (DM2_FLAG_NO_BACKWARD, DM2_FLAG_LEGACY_KERNELS): the per-pixel walk recomputes everything */
#define DM2_FWD_MASKS 2    /* per list entry the pixels it blended into: the backward re-clips those pairs exactly */
#define DM2_FWD_POOL 3     /* masks + pair pool: the default -- no clip for an area, Jacobians without a polygon */
#define DM2_FWD_POINT 4    /* aa_temperature == 0: per list entry the pixels whose rays hit it (point-sampled coverage) */

int dm2_abi_version(void);
const char* dm2_last_error(void);

/* Bytes of scratch of `kind` for `count` items (replaces required<T>(), state.h:63-69). */
size_t dm2_scratch_bytes(int kind, int64_t count, int64_t aux);

/* Bin faces into 16x16 tiles (preprocessFaceCUDA forward.cu:16-108) and count the
 * entries of every tile list; returns the number of (tile,face) pairs (`num_rendered`,
 * the reference's InclusiveSum of tiles_touched, renderer.cu:165-179) and the length of
 * the longest list (`max_tile_entries`, to be handed to dm2_forward_run), and `pair_bound`: an upper bound of
 * the (pixel, face) pairs the composite will look at (the faces' pixel rectangles inside the patch, summed) -- the
 * size of the pair pool a caller may append to the binning scratch (DM2_SCRATCH_PAIR_POOL).
 * Waits for the 16-byte read-back of those numbers. */
int dm2_forward_plan(const dm2_render_desc* d, void* face_scratch, size_t face_bytes,
                     void* stream, int64_t* num_rendered, int64_t* max_tile_entries, int64_t* pair_bound);

/* Per-tile lists ordered by (depth key, emission order) + tile ranges + per-pixel composite
 * (renderer.cu:185-266, FORWARD::renderCUDA forward.cu:139-432).  The lists are the ones the
 * reference's global stable radix sort of (tile | depth) keys produces; they are built by
 * bucketing the entries per tile and sorting every tile's segment on chip, unless
 * max_tile_entries > 32768 or DM2_FLAG_LEGACY_KERNELS asks for the radix route.
 * out_color (B,H,W,3), out_depth (B,H,W): written for every pixel.
 * out_tri_cnt (B,H,W) int32: number of AA records the reference would hold
 * (min(#overlapping faces visited, K)); may be NULL.  The face / binning / image
 * scratch must be kept (unmodified) for dm2_backward -- they are the three byte
 * buffers the reference returns and takes back (render.cu:194, render.h:79-81).
 * The face scratch holds a packed copy of the per-face inputs as the forward saw
 * them; the backward differentiates with respect to those.
 * Pair pool: when binning_bytes >= DM2_SCRATCH_BINNING bytes + DM2_SCRATCH_PAIR_POOL bytes for pair_bound, the
 * composite also leaves the coverage ratio (forward.cu:375-378) of every blended pair in the appended part and
 * *forward_mode is DM2_FWD_POOL; otherwise DM2_FWD_MASKS (a caller that finds pair_bound too large for its memory
 * simply appends nothing), DM2_FWD_POINT at aa_temperature 0, or DM2_FWD_NONE under DM2_FLAG_NO_BACKWARD /
 * DM2_FLAG_LEGACY_KERNELS.  forward_mode may be NULL.
 * out_face_weights (B,F) float32 or NULL (not wanted: the composite without that work runs); the caller zero-fills it (as the
 * gradient outputs of dm2_backward).  The composite adds, for every blend of face f into a pixel of view b's patch,
 * alpha * T -- the face's alpha there times the transmittance in front of it, the factor its colour gets in C += c alpha T
 * -- to out_face_weights[b * F + f].  So sum_f out_face_weights[b, f] = sum over the patch of 1 - T_final.  Float atomics:
 * the last bits may vary from run to run.  A caller that composites twice into the same weights (dm2_forward_run after a
 * dm2_forward that returned 0) must zero them in between. */
int dm2_forward_run(const dm2_render_desc* d, int64_t num_rendered, int64_t max_tile_entries, int64_t pair_bound,
                    void* face_scratch, size_t face_bytes,
                    void* binning_scratch, size_t binning_bytes,
                    void* image_scratch, size_t image_bytes,
                    float* out_color, float* out_depth, int32_t* out_tri_cnt, float* out_face_weights, void* stream,
                    int32_t* forward_mode);

/* dm2_forward_plan + dm2_forward_run in ONE call for a caller that already holds a binning scratch of plausible size (a
 * training loop: last frame's size plus headroom): the run step is enqueued straight from the plan's read-back, without
 * the round trip through the caller that otherwise leaves the GPU idle (~15 us of a 25-us gap through Python).
 * Returns 0 (rendered; *num_rendered / *max_tile_entries / *pair_bound / *forward_mode set), 2 when binning_bytes is
 * smaller than dm2_scratch_bytes(DM2_SCRATCH_BINNING, *num_rendered, B*tiles) + dm2_scratch_bytes(DM2_SCRATCH_PAIR_POOL,
 * *pair_bound, 0) -- the plan is done and nothing else: allocate and call dm2_forward_run -- or 1 on error.  A
 * larger-than-needed binning scratch is fine, also for dm2_backward (which must be given the same size).  out_tri_cnt,
 * out_face_weights and forward_mode may be NULL, as for dm2_forward_run; pair_bound must not. */
int dm2_forward(const dm2_render_desc* d, void* face_scratch, size_t face_bytes,
                void* binning_scratch, size_t binning_bytes, void* image_scratch, size_t image_bytes,
                float* out_color, float* out_depth, int32_t* out_tri_cnt, float* out_face_weights, void* stream,
                int64_t* num_rendered, int64_t* max_tile_entries, int64_t* pair_bound, int32_t* forward_mode);

/* Gradients (BACKWARD::renderCUDA backward.cu:17-532).  The six outputs must be
 * zero-filled by the caller (the reference's zeros_like, render.cu:313-318):
 * dL_dverts (P,3), dL_dverts_color (P,3), dL_dfaces_opacity (F),
 * dL_dverts_ndc (B,P,3) [only z written], dL_dfaces_intense (B,F),
 * dL_daa_face_verts (B,F,3,2).
 * forward_mode: what the forward of this frame returned (DM2_FWD_*; DM2_FWD_UNKNOWN costs a few idle launches).
 * tie_scratch: needed with DM2_FWD_POOL (and, when the binning scratch has a pool part, with DM2_FWD_UNKNOWN or
 * DM2_FWD_POINT at aa_temperature > 0):
 * dm2_scratch_bytes(DM2_SCRATCH_TIE_QUEUE, pairs of the pool part, 0) bytes, scratch of this call only.  The binning
 * scratch is not const: the pool backward keeps its queue counters there (left as it found them).
 * dL_dout_alpha (B,H,W) or NULL (zero: the kernels without that term run): the upstream gradient of the alpha image of
 * dm2_forward_alpha.  It reaches dL_dfaces_opacity and, through the AA coverage, dL_daa_face_verts (or verts_image); nothing
 * else. */
int dm2_backward(const dm2_render_desc* d, int64_t num_rendered, int32_t forward_mode,
                 const float* dL_dout_color, const float* dL_dout_depth, const float* dL_dout_alpha,
                 const void* face_scratch, size_t face_bytes,
                 void* binning_scratch, size_t binning_bytes,
                 const void* image_scratch, size_t image_bytes,
                 void* tie_scratch, size_t tie_bytes,
                 float* dL_dverts, float* dL_dverts_color, float* dL_dfaces_opacity,
                 float* dL_dverts_ndc, float* dL_dfaces_intense, float* dL_daa_face_verts,
                 void* stream);

/* The alpha (coverage) image of a forward: out_alpha (B,H,W) = 1 - T, the T the forward multiplied the background by
 * (0 where no face blended).  image_scratch: the forward's, unmodified.  Call it behind dm2_forward / dm2_forward_run
 * on the same stream; it reads nothing else. */
int dm2_forward_alpha(const dm2_render_desc* d, const void* image_scratch, size_t image_bytes, float* out_alpha, void* stream);

/* LayeredRenderer (render.h:101-119). */
typedef struct dm2_layers_desc {
    int32_t B, P, F, T;
    int32_t W, H, L;              /* full frame (with a dm2_window: the window's) width/height, num_layers */
    int32_t flags;                /* DM2_FLAG_ANALYTIC_RAYS, DM2_FLAG_LEGACY_KERNELS */
    const float* verts;           /* (P,3) */
    const int32_t* faces;         /* (F,3) */
    const int32_t* tets;          /* (T,4) */
    const int32_t* face_tets;     /* (F,2), -1 = none */
    const int32_t* tet_faces;     /* (T,4) */
    const int32_t* face_existence;/* (F) */
    const float* verts_ndc;       /* (B,P,3) */
    const float* verts_image;     /* (B,P,2) */
    const float* image_ray_o;     /* (B,H,W,3); may be NULL with DM2_FLAG_ANALYTIC_RAYS */
    const float* image_ray_d;     /* (B,H,W,3); may be NULL with DM2_FLAG_ANALYTIC_RAYS */
    const float* ray_cam;         /* DM2_FLAG_ANALYTIC_RAYS: (B,32), see dm2_render_desc */
} dm2_layers_desc;

/* A render window on the deferred path: dm2_layers_plan / dm2_layers_run / dm2_rasterize_* / dm2_coverage* /
 * dm2_layers_composite* take one next to the op's descriptor, whose W, H (and the H, W of dm2_coverage) are then the WINDOW's
 * size, as in dm2_render_desc, and every (B,H,W,...) array is the window's.  Pixel (x, y)
 * of view b's window is pixel (x + patch_min[b][0], y + patch_min[b][1]) of that view's full_W x full_H frame: its ray is that
 * frame pixel's (the ray tensors, when given, are the window's own (B,H,W,3) cut of the frame's; DM2_FLAG_ANALYTIC_RAYS
 * evaluates the absolute pixel with full_W, full_H), its pixel square for the coverage is the frame pixel's, and the 16 x 16
 * tile grid is anchored at the window's origin (patch_min), as dm2_forward_plan anchors it.  verts_image stays in the full
 * frame's pixel units.  The window must lie inside the frame (the caller checks: patch_min is device memory); the views may
 * have different origins.  patch_min NULL: every origin is (0, 0).  A NULL window pointer: the full frame of the descriptor's
 * W x H at origin 0.  Gradients add into the same outputs with and without a window. */
typedef struct dm2_window {
    const int32_t* patch_min;     /* (B,2) int32 (x, y) per view, DEVICE memory; NULL = zeros */
    int32_t full_W, full_H;       /* the frame the cameras' rays and verts_image belong to (Renderer.width/height) */
} dm2_window;

/* Bin the faces into the tiles of the frame, or of the window (win NULL: the full frame; otherwise the bbox of verts_image
 * against tiles anchored at patch_min); num_rendered / max_tile_entries as for dm2_forward_plan. */
int dm2_layers_plan(const dm2_layers_desc* d, const dm2_window* win, void* face_scratch, size_t face_bytes,
                    void* stream, int64_t* num_rendered, int64_t* max_tile_entries);
/* render_layers (B,H,W,L) must be pre-filled with -1 and render_layers_cnt (B,H,W)
 * with 0 by the caller (render.cu:437-438).  tet_scratch (DM2_SCRATCH_LAYER_TETS bytes for T tets; scratch of this call
 * only) receives one packed 256-B record per tet -- face vertices, outward normals, neighbours, existence flags -- so
 * that a step of the tet walk (forward.cu:853-996) is one contiguous fetch; NULL (or DM2_FLAG_LEGACY_KERNELS) selects the
 * reference's access pattern.  Same layers either way.  win (NULL: the full frame): the one the plan was given; the first-hit
 * pass and the tet walks run over the window's pixels with the window's rays. */
int dm2_layers_run(const dm2_layers_desc* d, const dm2_window* win, int64_t num_rendered, int64_t max_tile_entries,
                   void* face_scratch, size_t face_bytes,
                   void* binning_scratch, size_t binning_bytes,
                   void* image_scratch, size_t image_bytes,
                   void* tet_scratch, size_t tet_bytes,
                   int32_t* render_layers, int32_t* render_layers_cnt, void* stream);

/* Renderer.rasterize: the first L faces each pixel's ray hits, on any triangle mesh (no tetrahedra), with barycentrics and
 * ray parameter.  Plan with dm2_layers_plan (T = 0; tets, face_tets, tet_faces unused and may be NULL) and size the face /
 * binning / image scratch as for dm2_layers_run (the image scratch: DM2_SCRATCH_LAYER_IMAGE).  Per pixel (x, y) of view b
 * of the full frame, with its ray (image_ray_o / image_ray_d, or DM2_FLAG_ANALYTIC_RAYS):
 *   candidates: the faces of the pixel's tile list -- the face's verts_image bbox touches the tile and the NDC depth cull
 *     (max_z < -1 || min_z > 1) keeps it -- minus those with face_existence[f] == 0 (face_existence NULL: none dropped);
 *   hit: ray_tri_intersection(ro, rd, p0, p1, p2) succeeds with t >= 0, u >= 0, v >= 0, u + v <= 1 (p_k = verts[faces[f][k]])
 *     and the ray is off the face's plane: with E1 = p1 - p0, E2 = p2 - p0, n = cross(E1, E2), dn = dot(rd, n),
 *         dn * dn > (2.5e-7f * dot(n, n)) * dot(rd, rd)          (|cos(rd, n)| > 5e-4)
 *     in fp32, cross and dot as in ray_tri_intersection (dot = (x x + y y) + z z), the products in the order written, no
 *     contraction.  For a ray in the plane Moeller-Trumbore's denom is rounding noise that is seldom exactly 0, and t, u, v
 *     are noise that can pass the inside test at any t; above the bound denom holds its value to about 1e-7 / 5e-4 of
 *     itself.  A face of zero area (n == 0) is never hit;
 *   order: ascending (t, f); the first L hits are listed.
 * render_layers (B,H,W,L) int32 face ids, -1 = empty (the layout of dm2_layers_run, so they can go to dm2_layers_composite);
 * render_layers_cnt (B,H,W) int32 = hits listed (<= L); bary (B,H,W,L,3) float32 = (1 - u - v, u, v), the weights of
 * faces[f][0..2] (perspective-correct: from the world-space ray); t (B,H,W,L) float32 = the hit's ray parameter.  Empty
 * slots hold -1 in all three.  Every slot is written: no pre-fill.  fp32 in ray_tri_intersection's operation order, bit-exact.
 * The kernels stop a pixel's walk over its list (ordered by min depth) once a face's min depth lies beyond the largest max
 * depth of the L hits held: exact unless a face crosses the camera plane, as in dm2_layers_run's first-hit pass (the stop
 * relies on a hit's t lying within its face's depth range, which the off-plane rule secures).  A face that crosses the
 * camera plane may also be missing from the lists altogether, not only reordered: its vertices behind the camera project
 * mirrored, and the bbox of those projections, which the plan bins by, need not touch the tiles the face is seen in
 * (tests/tet_scenes.py "inside", 75 x 53, two cameras in the mesh: 1 181 of 6 901 clear float64 hits on such faces are in no
 * list).  dm2_rasterize_backward takes the caller's lists as they are; its only guard is rd . n == 0 exactly.
 * win (NULL: the full frame; plan with the same one): every array is (B,H,W,...) of the window.  The candidates of a window
 * pixel are the faces whose image bbox touches the pixel's 16 x 16 WINDOW tile (the grid anchored at patch_min) and that the
 * depth cull keeps; the hit rule, the (t, f) order, the early exit and the -1 of empty slots are as above, word for word, at
 * the frame pixel's ray.  A face that reaches a pixel through its bbox alone can therefore be a candidate under one grid and
 * not under another: a window and the crop of the full frame agree wherever the tiles coincide (origin a multiple of 16) and
 * may differ only in hits whose bbox misses one of the two tiles.
 * overlap == 0: the above; `inside` is not looked at and may be NULL.
 * overlap != 0 (Renderer.rasterize(overlap=True)): the faces that overlap a pixel's SQUARE, not only those its centre ray hits
 * -- the faces dm2_forward blends at a temperature > 0 (forward.cu:325-381), so that the deferred path draws a silhouette as it
 * does.  Plan, scratch, candidates (tile list, existence filter) and window rules are the same; d->verts_image must be given,
 * and inside must not be NULL unless L == 0.  A candidate f is listed at pixel (x, y) of view b iff
 *   (a) it overlaps the pixel: for the triangle verts_image[b, faces[f]], CCW-reordered, its tables built as under
 *       DM2_FLAG_TABLES_FROM_IMAGE, and the square [X, X+1] x [Y, Y+1], (X, Y) = (x, y) + patch_min[b], the clipper of dm2_coverage
 *       reports no error and area != 0 (so dm2_coverage of a listed slot is never 0 because the face misses the pixel);
 *   (b) ray_tri_intersection succeeds and the ray is off the face's plane (the rule above);
 *   (c) the slot's t (below) is >= 0.
 * Per listed slot, with (u, v) the intersection's and (uc, vc, code) = clamp_bary_uv(u, v) (auxiliary.h:292-329):
 *   bary = (1 - uc - vc, uc, vc);   inside = (code == 0), one byte, 1 or 0;
 *   t = the intersection's t when code == 0 (exactly the value of overlap == 0), otherwise the ray parameter of the clamped
 *       point's projection onto the ray, in fp32 in this order, without contraction (dot = (x x + y y) + z z):
 *         b0 = (1 - uc) - vc;  d_k = dot(p_k - ro, rd);  t = ((b0 * d0 + uc * d1) + vc * d2) / dot(rd, rd)
 *       (continuous across the triangle's edge, where the clamped point is the hit).
 * Order: ascending (t, f); the first L are listed; empty slots hold -1 in render_layers, bary and t and 0 in inside.  A slot
 * with inside == 1 is exactly a hit of overlap == 0: restricted to those slots, in order, the outputs are that call's
 * wherever neither list is truncated.  The walk over a pixel's list is exhaustive (no depth-bound stop: an off-triangle
 * slot's t is not a point of the ray on the face).  inside (B,H,W,L) uint8; every slot of every output is written. */
int dm2_rasterize_run(const dm2_layers_desc* d, const dm2_window* win, int64_t num_rendered, int64_t max_tile_entries,
                      void* face_scratch, size_t face_bytes,
                      void* binning_scratch, size_t binning_bytes,
                      void* image_scratch, size_t image_bytes,
                      int32_t* render_layers, int32_t* render_layers_cnt, float* bary, float* t,
                      int32_t overlap, uint8_t* inside, void* stream);
/* Gradients of dm2_rasterize_run's bary and t w.r.t. verts: dL_dverts (P,3), zero-filled by the caller.  For every slot of
 * render_layers with 0 <= f < F, upstream g = dL_dbary[slot] (3) and g_t = dL_dt[slot]:
 *   dL/dp_k += (g1 - g0) du/dp_k + (g2 - g0) dv/dp_k + g_t dt/dp_k,   p_k = verts[faces[f][k]],
 * at the pixel's ray.  Either upstream gradient may be NULL (zero; both NULL: nothing to do).  Nothing flows through the ray
 * or through which faces are listed.  Float atomics: the last bits may vary from run to run.  win (NULL: the full frame): the
 * forward's; the backward intersects again with the window's rays.
 * overlap != 0: render_layers are the lists of dm2_rasterize_run with overlap != 0.  Per slot with 0 <= f < F the intersection
 * and its clamp code are recomputed in fp32 as the forward computed them; with the code held fixed dL/d(uc, vc) =
 * (g1 - g0, g2 - g0) (+ g_t dt/d(uc, vc) where code != 0) goes through clamp_bary_uv_grad(code) to (u, v) and on to the
 * vertices as above; g_t goes through the intersection's t (code 0) or through the projection formula, its dependence on bary
 * included.  Nothing flows through the rays, the listing decision or inside. */
int dm2_rasterize_backward(const dm2_layers_desc* d, const dm2_window* win, const int32_t* render_layers, const float* dL_dbary,
                           const float* dL_dt, float* dL_dverts, int32_t overlap, void* stream);

/* Renderer.interpolate: attribute images from face ids and barycentrics per slot (dm2_rasterize_run's, dm2_layers_run's or
 * hand-built).  render_layers (B,H,W,L) int32, bary (B,H,W,L,3) float32, attr (N,C) float32 shared by the views
 * (view_tables == 0) or (B,N,C), one table per view (view_tables != 0), attr_faces (F,3) int32 rows of attr, out (B,H,W,L,C).
 * A slot s is filled when f = render_layers[s] lies in [0, F) and v_k = attr_faces[f][k], k = 0..2, all lie in [0, N):
 *   out[s,c] = (bary[s,0] * attr[v_0,c] + bary[s,1] * attr[v_1,c]) + bary[s,2] * attr[v_2,c]
 * in fp32, in this order, without contraction (bit-exact).  Every other slot is empty: out[s,:] = 0, and neither its bary
 * nor any attr row is read through it.  Every element of out is written: no pre-fill.  C >= 1; B * N < 2^31.
 * Launch bounds, forward and backward alike (refused with "interpolate: too many slots, rows or views", nothing launched):
 * B <= 65535; H <= 16 * 65535 (the tile rows of the attr backward's grid); ceil(B * H * W * L / 256) < 2^31. */
int dm2_interpolate(int32_t B, int32_t H, int32_t W, int32_t L, int32_t F, int32_t N, int32_t C, int32_t view_tables,
                    const int32_t* render_layers, const float* bary, const float* attr, const int32_t* attr_faces,
                    float* out, void* stream);
/* Gradients of dm2_interpolate for upstream g = dL_dout (B,H,W,L,C).  Per filled slot s:
 *   dL_dattr[v_k,c] += bary[s,k] * g[s,c]   (the view's table when view_tables != 0); dL_dattr is zero-filled by the caller;
 *   dL_dbary[s,k] = sum_c attr[v_k,c] * g[s,c]; 0 in an empty slot; every element is written.
 * Either output pointer may be NULL (not wanted; its kernel is not launched).  dL_dattr is summed with float atomics: its
 * last bits may vary from run to run; dL_dbary is a pure function of the inputs. */
int dm2_interpolate_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t F, int32_t N, int32_t C, int32_t view_tables,
                             const int32_t* render_layers, const float* bary, const float* attr, const int32_t* attr_faces,
                             const float* dL_dout, float* dL_dattr, float* dL_dbary, void* stream);

/* Renderer.texture: a texture sampled at per-slot UVs (dm2_interpolate's output for a 2-channel attribute, or hand-built).
 * uv (B,H,W,L,2) float32 = (u, v), u along the texture's width; tex (Ht,Wt,C) float32 shared by the views
 * (view_textures == 0) or (B,Ht,Wt,C), one texture per view (view_textures != 0), channel-last; render_layers (B,H,W,L) int32
 * or NULL; out (B,H,W,L,C).  Ht, Wt, C >= 1; Ht * Wt < 2^31.  Texel centres sit at ((i + 0.5) / Wt, (j + 0.5) / Ht).  Per slot
 * s, all fp32, separate multiplies and adds in the written order, without contraction (bit-exact):
 *   x  = u * (float)Wt - 0.5f         y  = v * (float)Ht - 0.5f
 *   x0 = floorf(x)   fx = x - x0       y0 = floorf(y)   fy = y - y0
 * A slot is empty when render_layers[s] < 0 (render_layers NULL: never by id), or u or v is not finite, or |x| or |y| is not
 * below 2^24: out[s,:] = 0, and nothing is read from tex through it.  Otherwise i0 = (int)x0, i1 = i0 + 1, j0 = (int)y0,
 * j1 = j0 + 1, addressed per boundary mode: DM2_TEX_BOUNDARY_WRAP addr(i) = ((i % n) + n) % n, DM2_TEX_BOUNDARY_CLAMP
 * addr(i) = min(max(i, 0), n - 1), n = Wt for columns and Ht for rows; t_pq = tex[addr(j0 + q)][addr(i0 + p)]:
 *   DM2_TEX_FILTER_LINEAR   a = t00 + fx * (t10 - t00), b = t01 + fx * (t11 - t01), out[s,c] = a + fy * (b - a)
 *   DM2_TEX_FILTER_NEAREST  out[s,c] = tex[addr((int)floorf(y + 0.5f))][addr((int)floorf(x + 0.5f))]
 * Every element of out is written: no pre-fill. */
#define DM2_TEX_FILTER_NEAREST 0
#define DM2_TEX_FILTER_LINEAR 1
#define DM2_TEX_BOUNDARY_WRAP 0
#define DM2_TEX_BOUNDARY_CLAMP 1
int dm2_texture(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t view_textures,
                int32_t filter, int32_t boundary, const int32_t* render_layers, const float* uv, const float* tex, float* out,
                void* stream);
/* Gradients of dm2_texture for upstream g = dL_dout (B,H,W,L,C): the derivative of the fp32 function above at its fp32 fx, fy
 * and addresses.  Per non-empty slot s:
 *   dL_dtex[t_pq,c] += w_pq * g[s,c], w = ((1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy)  (nearest: weight 1 on the one texel); the
 *     view's own texture when view_textures != 0, summed over the views otherwise; two corners that address one texel (clamp
 *     at a border, wrap at n = 1) both add; dL_dtex is zero-filled by the caller;
 *   dL_duv[s,0] = Wt * sum_c g[s,c] * ((t10 - t00) + fy * ((t11 - t01) - (t10 - t00))),  dL_duv[s,1] = Ht * sum_c g[s,c] * (b - a)
 *     (used as it stands where clamp has a kink); zeros for nearest and in an empty slot; every element is written.
 * Either output pointer may be NULL (not wanted; its kernel is not launched; tex may then be NULL for dL_dtex alone).
 * dL_dtex is summed with float atomics: its last bits may vary from run to run; dL_duv is a pure function of the inputs. */
int dm2_texture_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t view_textures,
                         int32_t filter, int32_t boundary, const int32_t* render_layers, const float* uv, const float* tex,
                         const float* dL_dout, float* dL_dtex, float* dL_duv, void* stream);

/* Renderer.texture(boundary_mode="cube"): a cube map looked up by a direction per slot.  dirs (B,H,W,L,3) float32, any
 * non-zero length (dm2_interpolate's output for a 3-channel attribute such as a normal, or hand-built); tex (6,N,N,C) float32
 * shared by the views (view_textures == 0) or (B,6,N,N,C), one cube per view, channel-last, faces in the order +x, -x, +y, -y,
 * +z, -z; render_layers (B,H,W,L) int32 or NULL; out (B,H,W,L,C).  N, C >= 1; 6 * N * N < 2^31.  filter: DM2_TEX_FILTER_*.
 * A slot is empty when render_layers[s] < 0 (render_layers NULL: never by id), or a component of the direction is not finite,
 * or all three are zero: out[s,:] = 0, and nothing is read from tex through it.  Otherwise, per slot s with direction
 * (x, y, z), all fp32, separate multiplies and adds in the written order, without contraction (bit-exact):
 *   ax = |x|, ay = |y|, az = |z|;  the major axis is x if ax >= ay && ax >= az, else y if ay >= az, else z;
 *   face = 2 * axis + (1 if the major component is negative);  ma = |major component|;  (sc, tc) by the OpenGL table:
 *     +x: (-z, -y)   -x: (+z, -y)   +y: (+x, +z)   -y: (+x, -z)   +z: (+x, -y)   -z: (-x, -y)
 *   sn = 0.5f * (sc / ma + 1.0f)       tn = 0.5f * (tc / ma + 1.0f)
 *   X  = sn * (float)N - 0.5f          Y  = tn * (float)N - 0.5f              (both in [-0.5, N - 0.5])
 *   X0 = floorf(X)   fx = X - X0       Y0 = floorf(Y)   fy = Y - Y0
 *   DM2_TEX_FILTER_NEAREST  out[s,c] = tex[face][clamp((int)floorf(Y + 0.5f))][clamp((int)floorf(X + 0.5f))],
 *     clamp(i) = min(max(i, 0), N - 1)
 *   DM2_TEX_FILTER_LINEAR   taps (i0 + p, j0 + q), i0 = (int)X0, j0 = (int)Y0, tap k = p + 2 q, t_k its texel:
 *     a tap inside the face is tex[face][j][i];
 *     a tap outside on exactly one axis lies beyond border e of the face (0: i < 0, 1: i >= N, 2: j < 0, 3: j >= N) at position
 *       k' = j (borders 0, 1) or i (borders 2, 3) along it, and is the texel of the face across that edge, in that face's
 *       column or row along the shared edge, at the same position along the edge: with (nf, ne, rev) = SEAM[face][e] and
 *       k'' = rev ? N - 1 - k' : k', tex[nf][k''][0] for ne == 0, tex[nf][k''][N - 1] for ne == 1, tex[nf][0][k''] for ne == 2,
 *       tex[nf][N - 1][k''] for ne == 3;  SEAM[6][4] =
 *         +x: {+z,1,0} {-z,0,0} {+y,1,1} {-y,1,0}     -x: {-z,1,0} {+z,0,0} {+y,0,0} {-y,0,1}
 *         +y: {-x,2,0} {+x,2,1} {-z,2,1} {+z,2,0}     -y: {-x,3,1} {+x,3,0} {+z,3,0} {-z,3,1}
 *         +z: {-x,1,0} {+x,0,0} {+y,3,0} {-y,2,0}     -z: {+x,1,0} {-x,0,0} {+y,2,1} {-y,3,1}
 *     a tap outside on both axes (a cube corner) does not exist; at most one tap of a sample is such a tap.
 *     With all four taps: a = t0 + fx * (t1 - t0), b = t2 + fx * (t3 - t2), out[s,c] = a + fy * (b - a)   (dm2_texture's blend).
 *     With tap m missing: gx = 1.0f - fx, gy = 1.0f - fy, w = (gx * gy, fx * gy, gx * fy, fx * fy) with w_m = 0 and t_m = 0,
 *       W = ((w0 + w1) + w2) + w3   (>= 0.75: the missing weight is at most 0.25),
 *       out[s,c] = (((w0 * t0 + w1 * t1) + w2 * t2) + w3 * t3) / W.
 * Every element of out is written: no pre-fill. */
int dm2_texture_cube(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures, int32_t filter,
                     const int32_t* render_layers, const float* dirs, const float* tex, float* out, void* stream);
/* Gradients of dm2_texture_cube for upstream g = dL_dout (B,H,W,L,C): the derivative of the fp32 function above at its fp32
 * fractions, faces and addresses.  Per non-empty slot s:
 *   dL_dtex[t_k,c] += w_k * g[s,c], w = ((1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy), at a corner w_k / W over the three taps that
 *     exist (nearest: weight 1 on the one texel); the view's own cube when view_textures != 0, summed over the views otherwise;
 *     two taps that address one texel (N = 1) both add; dL_dtex is zero-filled by the caller;
 *   dL_ddir[s] goes through fx, fy (d out / d fx = (t1 - t0) + fy * ((t3 - t2) - (t1 - t0)), d out / d fy = b - a; at a
 *     corner sum_k (dw_k / dfx) * (t_k - out) / W and alike for fy), then X = sn * N - 0.5, sn = 0.5 * (u + 1), u = sc / ma
 *     (d/dsc = 1 / ma, d/dma = -sc / ma^2), tn alike, and the signs of the table; it is orthogonal to the direction (the lookup
 *     does not depend on the length); zeros for nearest and in an empty slot; every element is written.
 * Either output pointer may be NULL (not wanted; its kernel is not launched; tex may then be NULL for dL_dtex alone).
 * dL_dtex is summed with float atomics: its last bits may vary from run to run; dL_ddir is a pure function of the inputs. */
int dm2_texture_cube_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures,
                              int32_t filter, const int32_t* render_layers, const float* dirs, const float* tex,
                              const float* dL_dout, float* dL_dtex, float* dL_ddir, void* stream);

/* Renderer.texture3d: a voxel grid looked up by a position per slot.  xyz (B,H,W,L,3) float32, the position in the grid's unit
 * cube, x along the grid's last spatial axis and z along its first; grid (N,N,N,C) float32 shared by the views
 * (view_textures == 0) or (B,N,N,N,C), channel-last, indexed [k][j][i]; render_layers (B,H,W,L) int32 or NULL; out (B,H,W,L,C).
 * N, C >= 1; N * N * N < 2^31.  filter: DM2_TEX_FILTER_*; boundary: DM2_TEX_BOUNDARY_WRAP or DM2_TEX_BOUNDARY_CLAMP; any other
 * filter or boundary is refused.
 * Voxel centres sit at ((i + 0.5) / N, (j + 0.5) / N, (k + 0.5) / N).  Per slot s, all fp32, separate multiplies and adds in
 * the written order, without contraction (bit-exact):
 *   X  = x * (float)N - 0.5f      Y = y * (float)N - 0.5f      Z = z * (float)N - 0.5f
 *   X0 = floorf(X)   fx = X - X0   i0 = (int)X0                 (Y0, fy, j0 and Z0, fz, k0 alike)
 * A slot is empty when render_layers[s] < 0 (render_layers NULL: never by id), or a coordinate is not finite, or |X|, |Y| or |Z|
 * is not below 2^24 (dm2_texture's rule, per axis): out[s,:] = 0, and nothing is read from the grid through it.  Otherwise the
 * eight taps are t_pqr = grid[addr(k0 + r)][addr(j0 + q)][addr(i0 + p)] with dm2_texture's addr of the boundary, n = N:
 *   DM2_TEX_FILTER_LINEAR   a_r = b0 + fy * (b1 - b0), b_q = t_0qr + fx * (t_1qr - t_0qr)   (dm2_texture's blend in plane k0 + r),
 *                           out[s,c] = a_0 + fz * (a_1 - a_0)
 *   DM2_TEX_FILTER_NEAREST  out[s,c] = grid[addr((int)floorf(Z + 0.5f))][addr((int)floorf(Y + 0.5f))][addr((int)floorf(X + 0.5f))]
 * Every element of out is written: no pre-fill. */
int dm2_texture_volume(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures, int32_t filter,
                       int32_t boundary, const int32_t* render_layers, const float* xyz, const float* grid, float* out, void* stream);
/* Gradients of dm2_texture_volume for upstream g = dL_dout (B,H,W,L,C): the derivative of that fp32 function at its fp32
 * fractions and addresses.  Per non-empty slot s:
 *   dL_dgrid[t_pqr,c] += w_pqr * g[s,c], w_pqr = (wx_p * wy_q) * wz_r with (w_0, w_1) = (1 - f, f) per axis (nearest: weight 1
 *     on the one voxel); the view's own grid when view_textures != 0, summed over the views otherwise; taps that meet in one
 *     voxel (N = 1, clamp at a border) all add; dL_dgrid is zero-filled by the caller and summed with float atomics: its last
 *     bits may vary from run to run;
 *   dL_dxyz[s,a] = (float)N * sum_c g[s,c] * d out / d f_a, with u_r = (t_10r - t_00r) + fy * ((t_11r - t_01r) - (t_10r - t_00r))
 *     and v_r = b1 - b0 of plane r:  d out / d fx = U_0 + fz * (U_1 - U_0),  d out / d fy = V_0 + fz * (V_1 - V_0) over the sums
 *     U_r = sum_c g * u_r, V_r = sum_c g * v_r, and d out / d fz = a_1 - a_0; used as it stands where clamp has a kink; zeros
 *     for nearest and in an empty slot; every element is written; a pure function of the inputs.
 * Either output pointer may be NULL (not wanted; its kernel is not launched; grid may then be NULL for dL_dgrid alone). */
int dm2_texture_volume_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures,
                                int32_t filter, int32_t boundary, const int32_t* render_layers, const float* xyz, const float* grid,
                                const float* dL_dout, float* dL_dgrid, float* dL_dxyz, void* stream);

/* Renderer.hash_grid: a multiresolution hash encoding looked up by a position per slot.  NL = num_levels, F = features,
 * T = 2^log2_rows rows per level, q = growth16 (growth q / 16): xyz (B,H,W,L,3) float32, the position in the field's unit cube,
 * axes as for the volume; table (NL, T, F) float32, shared by the views; render_layers (B,H,W,L) int32 or NULL; out and dL_dout
 * are (B,H,W,L,NL*F), level-major: channel l * F + f.  filter and boundary as for dm2_texture_volume.
 * Refused: NL outside 1..32; q outside 17..32; F not in {1, 2, 4, 8}; log2_rows outside 4..24; base_resolution < 1;
 * R_{NL-1} > 2^20; NL * T * F >= 2^31; B * NL > 65535; NULL xyz; an unknown filter or boundary.
 * Level resolutions, integers:  R_0 = base_resolution,  R_{l+1} = (R_l * q) >> 4.
 * One level l is the volume's lookup above of a virtual R_l^3 grid, n = R_l, whose voxel (k, j, i) is row row_l(k, j, i) of
 * table[l]; all fp32, separate multiplies and adds in the written order, without contraction (bit-exact):
 *   X  = x * (float)R_l - 0.5f   X0 = floorf(X)   fx = X - X0   i0 = (int)X0        (Y0, fy, j0 and Z0, fz, k0 alike)
 *   t_pqr = table[l][row_l(addr(k0 + r), addr(j0 + q), addr(i0 + p))]               (addr: the volume's, of the boundary)
 *   DM2_TEX_FILTER_LINEAR   out[s, l*F + f] = a_0 + fz * (a_1 - a_0), a_r the volume's blend of plane k0 + r
 *   DM2_TEX_FILTER_NEAREST  out[s, l*F + f] = table[l][row_l(addr((int)floorf(Z + 0.5f)), addr(.. Y ..), addr(.. X ..))]
 * Row addressing, on the addresses after addr:
 *   (int64)R_l^3 <= T (a dense level):  row = (k * R_l + j) * R_l + i
 *   otherwise, in uint32_t arithmetic that wraps:  row = (i ^ (j * 2654435761u) ^ (k * 805459861u)) & (T - 1)
 * Taps that land in one row (collisions, R_l = 1, clamp at a border) all read it, and all add to it in the backward.
 * A slot is empty when render_layers[s] < 0 (render_layers NULL: never by id), or |X|, |Y| or |Z| at the finest level l = NL - 1
 * is not below 2^24 (NaN and infinities included; the R_l do not decrease, so no coarser level is out of range when the finest
 * is not): zeros in all NL * F channels, nothing read from the table through it, no gradient.  Every element of out is written. */
int dm2_hash_grid(int32_t B, int32_t H, int32_t W, int32_t L, int32_t base_resolution, int32_t log2_rows, int32_t num_levels,
                  int32_t features, int32_t growth16, int32_t filter, int32_t boundary, const int32_t* render_layers, const float* xyz,
                  const float* table, float* out, void* stream);
/* Gradients of dm2_hash_grid for upstream g = dL_dout: the derivative of that fp32 function at its fp32 fractions and addresses.
 *   dL_dtable[l, row_pqr, f] += ((wx_p * wy_q) * wz_r) * g[s, l*F + f], (w_0, w_1) = (1 - f, f) per axis (nearest: weight 1 on
 *     the one row); zero-filled by the caller, summed with float atomics: its last bits may vary from run to run;
 *   dL_dxyz[s, a] = sum over l = 0 .. NL - 1, in that order from 0.0f, of (float)R_l * the level's volume term:
 *     U_0 + fz * (U_1 - U_0), V_0 + fz * (V_1 - V_0) and sum_f g * (a_1 - a_0), the sums over the level's F features in order
 *     (the volume's U_r, V_r); zeros for nearest and in an empty slot; every element is written; a pure function of the inputs.
 * Either output pointer may be NULL (not wanted; its kernel is not launched; table may then be NULL for dL_dtable alone). */
int dm2_hash_grid_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t base_resolution, int32_t log2_rows, int32_t num_levels,
                           int32_t features, int32_t growth16, int32_t filter, int32_t boundary, const int32_t* render_layers,
                           const float* xyz, const float* table, const float* dL_dout, float* dL_dtable, float* dL_dxyz, void* stream);

/* Renderer.bary_derivatives: the footprint of a pixel on each listed face.  render_layers (B,H,W,L) int32, verts (P,3) float32,
 * faces (F,3) int32, ray_cam (B,32) float32 = inv(mv) (16, row-major) then inv(proj) (16) of each view, the camera block of
 * DM2_FLAG_ANALYTIC_RAYS; dbary_dx, dbary_dy (B,H,W,L,3) float32 = the derivatives of the slot's perspective-correct barycentrics
 * (1 - u - v, u, v) (dm2_rasterize_run's bary, unclamped) with respect to the pixel's x and y position in pixels.  The layout is
 * dm2_interpolate's bary: dm2_interpolate is linear in bary, so interpolating with dbary_dx gives d(attribute)/dX.
 * The unnormalised ray direction is affine in the pixel position, and u, v do not change when it is scaled.  Per slot of
 * view b at window pixel (x, y), frame pixel (X, Y) = (x, y) + patch_min[b] (win NULL: the full frame, full_W = W, full_H = H),
 * imv = ray_cam[b], ipr = ray_cam[b] + 16, all fp32, separate multiplies and adds in the written order, without contraction, dot =
 * (x x + y y) + z z, cross as in ray_tri_intersection (bit-exact):
 *   h    = (((X + 0.5f) / full_W * 2.0f) - 1.0f, ((Y + 0.5f) / full_H * 2.0f) - 1.0f, -1.0f, 1.0f)
 *   v_j  = ((h0 * ipr[4j] + h1 * ipr[4j+1]) + h2 * ipr[4j+2]) + h3 * ipr[4j+3],   j = 0..3
 *   w_k  = ((v0 * imv[4k] + v1 * imv[4k+1]) + v2 * imv[4k+2]) + v3 * imv[4k+3],   k = 0..2
 *   ro   = (imv[3], imv[7], imv[11]),   D = w - ro                          (analytic_ray's direction before it is normalised)
 *   gX_k = (2.0f / full_W) * (((imv[4k] * ipr[0] + imv[4k+1] * ipr[4]) + imv[4k+2] * ipr[8]) + imv[4k+3] * ipr[12])     (= dD/dX)
 *   gY_k = (2.0f / full_H) * (((imv[4k] * ipr[1] + imv[4k+1] * ipr[5]) + imv[4k+2] * ipr[9]) + imv[4k+3] * ipr[13])     (= dD/dY)
 *   T = ro - p0, E1 = p1 - p0, E2 = p2 - p0 (p_k = verts[faces[f][k]]),  a = cross(E2, T), b = cross(T, E1), c = cross(E2, E1)
 *   Dc = dot(D, c),  r = 1.0f / Dc (the one reciprocal),  u = dot(D, a) * r,  v = dot(D, b) * r
 *   du = (dot(gX, a) - u * dot(gX, c)) * r,  dv = (dot(gX, b) - v * dot(gX, c)) * r,  dbary_dx[s] = (-(du + dv), du, dv)
 * and dbary_dy likewise with gY.  A slot is empty when its id is outside [0, F) or its face names a vertex outside [0, P); an
 * empty slot and a slot with Dc == 0 give zeros.  The kernel reads neither ray tensors nor bary.  Every element of both
 * outputs is written.  No backward: the footprint is a constant of the pipeline. */
int dm2_bary_derivatives_window(int32_t B, int32_t H, int32_t W, int32_t L, int32_t P, int32_t F,
                                const dm2_window* win /* NULL: full frame */, const int32_t* render_layers, const float* verts,
                                const int32_t* faces, const float* ray_cam, float* dbary_dx, float* dbary_dy, void* stream);

/* Renderer.texture_mipmaps: the mip chain of NB textures tex (NB,Ht,Wt,C) float32 (NB = 1: a shared texture).  Level 0 is tex
 * itself and is not copied.  Level k+1 exists while both extents of level k are even and k < max_mip_level (max_mip_level < 0: no
 * limit); its extents are (H_k / 2, W_k / 2) and each texel is, in fp32 in this order,
 *   ((p00 + p10) + (p01 + p11)) * 0.25f,   p_pq = level_k[2j + q][2i + p]
 * nlev = 1 + the levels built (2048 x 2048: 12; 16 x 8: 4, ending at 2 x 1; 6 x 10: 2; 5 x 7: 1).  mip (NB,T,C): levels
 * 1 .. nlev-1 concatenated per texture, each (H_k, W_k, C) row-major; T = their texels (0 when nlev == 1: nothing runs).
 * Ht * Wt + T < 2^31.  Bit-exact; every element of mip is written. */
int dm2_texture_mipmaps(int32_t NB, int32_t Ht, int32_t Wt, int32_t C, int32_t max_mip_level, const float* tex, float* mip,
                        void* stream);
/* Gradient of dm2_texture_mipmaps for upstream dL_dmip (NB,T,C): every texel of dL_dtex (NB,Ht,Wt,C) is written as
 *   sum_{k = 1 .. nlev-1} 0.25^k * dL_dmip_k[j >> k][i >> k]      (acc = acc + w_k * g_k, k ascending)
 * a gather: no atomics, a pure function of the inputs (zeros when nlev == 1). */
int dm2_texture_mipmaps_backward(int32_t NB, int32_t Ht, int32_t Wt, int32_t C, int32_t max_mip_level, const float* dL_dmip,
                                 float* dL_dtex, void* stream);
/* Every non-negative max_mip_level of the two entry points above is a level limit.  (Up to ABI 7 bit 30 of it selected the
 * cube prefilter below; a caller built against that version is stopped by dm2_abi_version before it gets here.) */

/* Renderer.cube_prefilter: the GGX prefilter of cube mip chains.  x, y (cubes,6,T,C) float32: per cube its six faces (+x, -x,
 * +y, -y, +z, -z, dm2_texture_cube's face coordinates), per face the levels 1 .. nlev-1 of dm2_texture_mipmaps' layout for
 * (N, N, max_mip_level) (max_mip_level < 0: no limit); T == 0: nothing runs; 0 <= cubes <= 10922; 6 * (N * N + T) < 2^31;
 * 1 <= C <= 262140.  dm2_cube_prefilter_backward is the transpose: ybar, xbar of the same shape.
 * Texel (face, j, i) of a level with faces of n x n, all fp32, separate multiplies and adds in the written order:
 *   sc = (2 (i + 0.5)) / n - 1,  tc = (2 (j + 0.5)) / n - 1,  p = the cube point of (face, sc, tc) (the inverse of the lookup's table)
 *   q = (1 + sc sc) + tc tc,  rq = sqrtf(q),  d = p / rq per component,  Om = 1 / (q rq)   (the solid angle up to 4 / n^2)
 * Level k >= 1 (n = N >> k) has roughness r = (float)k / (float)(nlev - 1), a = r r, a2 = a a.  For texels o, s of that level:
 *   m = ((d_o.x - d_s.x)^2 + (d_o.y - d_s.y)^2) + (d_o.z - d_s.z)^2          (= 2 (1 - cos))
 *   c = 1 - 0.5 m,   e = a2 + (1 - a2) (0.25 m)                               (0.25 m = sin^2 of the half angle)
 *   member: c > 0 and e <= 64 a2;   K(o,s) = ((a2 / e) (a2 / e)) c for a member, 0 otherwise
 * K = D(n.h) (n.l) of the split-sum GGX lobe with n = v = r, scaled to peak 1; symmetric in (o, s) to the bit; a texel is its
 * own member.  The cut drops the lobe below 1/4096 of its peak, at most 1/64 of the distribution's mass (its CDF is
 * a2 cos^2 / e); for a2 >= 1/127 it never bites, and at r = 1 K = c on the open hemisphere: the cosine lobe.  Each level is
 * filtered from the same level of the input, un-normalised:
 *   forward:   y[o,ch] = sum_s (K(o,s) Om_s) x[s,ch]          backward (the transpose): xbar[s,ch] = Om_s sum_o K(o,s) ybar[o,ch]
 * Both are gathers: every element is written, no atomics, a pure function of the inputs.  The order of the sums is the
 * kernel's own: against the sums in float64 an element with mem members is held to (mem + 4) 2^-24 sum |K Om x|. */
int dm2_cube_prefilter(int32_t cubes, int32_t N, int32_t C, int32_t max_mip_level, const float* x, float* y, void* stream);
int dm2_cube_prefilter_backward(int32_t cubes, int32_t N, int32_t C, int32_t max_mip_level, const float* ybar, float* xbar,
                                void* stream);

/* Renderer.texture(filter_mode="linear-mipmap-linear"): trilinear sampling.  uv, tex, render_layers, out, view_textures and
 * boundary as for dm2_texture; uv_da (B,H,W,L,4) float32 = (du/dX, dv/dX, du/dY, dv/dY), the UV footprint of the slot's pixel
 * (dm2_interpolate of dm2_bary_derivatives_window's outputs); mip: dm2_texture_mipmaps' chain of tex under the same
 * max_mip_level, (T,C) or, with view_textures, (B,T,C) (may be NULL when T == 0).  Per slot s, all fp32 in the written order:
 *   empty: the slot is empty by dm2_texture's rules evaluated at level 0, or any of its four uv_da is not finite:
 *     out[s,:] = 0, nothing is read from tex or mip through it, no gradient;
 *   footprint: ax = dudX * (float)Wt, bx = dvdX * (float)Ht, sx = ax * ax + bx * bx; sy likewise from (dudY, dvdY); r2 = max(sx, sy);
 *   level of detail: r2 <= 1: lod = 0; otherwise r2 = m * 2^e with m in [1, 2) read from the float's bits (e = the biased
 *     exponent - 127, m = the mantissa bits under exponent 0; r2 = infinity: e = 128, m = 1) and
 *         lod = 0.5f * ((float)e + (m - 1.0f))
 *     log2 with the mantissa taken linearly: no transcendental, so the forward is a pure function of IEEE operations.  lod never
 *     exceeds 0.5 log2(r2) and falls short of it by at most 0.5 (log2(1 / ln 2) - (1 / ln 2 - 1)) = 0.04304 levels;
 *   blend: lod <= 0: level 0 alone (bit-equal to DM2_TEX_FILTER_LINEAR); lod >= nlev - 1: the last level alone; otherwise
 *     j = (int)floorf(lod), f = lod - (float)j, out[s,c] = c_j + f * (c_{j+1} - c_j)
 *     c_k = dm2_texture's linear sample of level k: taps from x_k = u * (float)W_k - 0.5f, y_k = v * (float)H_k - 0.5f, the
 *     boundary mode's addressing with that level's extents, a + fy * (b - a).
 * Every element of out is written. */
int dm2_texture_mip(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t view_textures,
                    int32_t boundary, int32_t max_mip_level, const int32_t* render_layers, const float* uv, const float* uv_da,
                    const float* tex, const float* mip, float* out, void* stream);
/* Gradients of dm2_texture_mip for upstream g = dL_dout (B,H,W,L,C): the derivative of the fp32 function above at its own lod, j,
 * f, fractions and addresses.  The level of detail is a constant of the op: uv_da gets no gradient.  Per non-empty slot, with
 * (m_j, m_{j+1}) = (1 - f, f) (one level: weight 1 on it):
 *   dL_dtex / dL_dmip[t_pq of level k, c] += m_k * w_pq * g[s,c], w as in dm2_texture_backward: level 0's texels in dL_dtex
 *     (tex's shape), the others in dL_dmip (mip's shape); both zero-filled by the caller; float atomics;
 *   dL_duv[s] = m_j * duv_j + m_{j+1} * duv_{j+1},  duv_k = dm2_texture_backward's dL_duv of level k with its own W_k, H_k
 *     factors; zeros in an empty slot; every element is written; a pure function of the inputs.
 * Any of the three output pointers may be NULL (not wanted; a kernel none of whose outputs is wanted is not launched; tex and
 * mip may be NULL when dL_duv is). */
int dm2_texture_mip_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t view_textures,
                             int32_t boundary, int32_t max_mip_level, const int32_t* render_layers, const float* uv,
                             const float* uv_da, const float* tex, const float* mip, const float* dL_dout, float* dL_dtex,
                             float* dL_dmip, float* dL_duv, void* stream);

/* Renderer.texture(filter_mode="linear-mipmap-linear", boundary_mode="cube", mip_level=...): a cube map and its mip chain looked
 * up by a direction and a level of detail per slot.  dirs (B,H,W,L,3), render_layers, out and view_textures as for
 * dm2_texture_cube; level (B,H,W,L) float32, the level of detail, one float per slot, level 0 being tex; tex (6,N,N,C) or, with
 * view_textures, (B,6,N,N,C); mip (6,T,C) or (B,6,T,C): per face the levels 1 .. nlev-1 in dm2_texture_mipmaps' layout for
 * (N, N, max_mip_level) (max_mip_level < 0: no limit), level k with faces of N_k = N >> k (dm2_texture_mipmaps of the six faces
 * as six textures gives the box chain; any chain of that shape is accepted); 6 * (N * N + T) < 2^31; mip may be NULL when T == 0.
 *   empty: the slot is empty by dm2_texture_cube's rules, or its level is not finite: out[s,:] = 0, nothing is read through it,
 *     no gradient;
 *   lod = the slot's level, all fp32 in the written order: lod <= 0: level 0 alone (bit-equal to dm2_texture_cube
 *     with DM2_TEX_FILTER_LINEAR); lod >= nlev - 1: the last level alone; otherwise j = (int)floorf(lod), f = lod - (float)j,
 *       out[s,c] = c_j + f * (c_{j+1} - c_j)
 *     c_k = dm2_texture_cube's linear sample of level k with N_k in place of N: the face and (sc, tc, ma), and with them
 *     sn, tn, are computed once; X_k = sn * (float)N_k - 0.5f, Y_k alike; the seam rule and the three-tap corner blend apply at
 *     that level's size.
 * Every element of out is written. */
int dm2_texture_cube_mip(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures, int32_t max_mip_level,
                         const int32_t* render_layers, const float* dirs, const float* level, const float* tex, const float* mip,
                         float* out, void* stream);
/* Gradients of dm2_texture_cube_mip for upstream g = dL_dout (B,H,W,L,C): the derivative of that fp32 function at its own j, f,
 * fractions, faces and addresses, with (m_j, m_{j+1}) = (1 - f, f) (one level: weight 1 on it):
 *   dL_dtex / dL_dmip[t_k of level k, c] += m_k * w * g[s,c], w as in dm2_texture_cube_backward (w / W at a corner; a missing
 *     tap adds nothing): level 0's texels in dL_dtex, the others in dL_dmip; zero-filled by the caller; float atomics;
 *   dL_drows is (B,H,W,L,4) = (dL/ddir.x, .y, .z, dL/dlevel), one 16-byte row per slot (16-byte aligned), every element written:
 *     dL/ddir = m_j * ddir_j + m_{j+1} * ddir_{j+1}, ddir_k = dm2_texture_cube_backward's dL_ddir of level k with its N_k
 *       factor; orthogonal to the direction;
 *     dL/dlevel = sum_c g[s,c] * (c_{j+1,c} - c_{j,c}), the channels in order, where 0 < lod < nlev - 1 (at an integer lod
 *       inside the range the right-hand derivative, j = lod); 0 where the level is clamped or the slot is empty;
 *     a pure function of the inputs.
 * Any of the three output pointers may be NULL (not wanted; a kernel none of whose outputs is wanted is not launched; tex and
 * mip may be NULL when dL_drows is); dL_drows is produced when either the direction's or the level's gradient is wanted. */
int dm2_texture_cube_mip_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures,
                                  int32_t max_mip_level, const int32_t* render_layers, const float* dirs, const float* level,
                                  const float* tex, const float* mip, const float* dL_dout, float* dL_dtex, float* dL_dmip,
                                  float* dL_drows, void* stream);

/* Renderer.composite: per-slot values (dm2_interpolate's or dm2_texture's output, or anything shaded from them) blended front
 * to back into an image: LayeredRenderer.render's blend with the colour supplied by the caller.
 * values (B,H,W,L,C) float32, C >= 1; alpha float32: (B,H,W,L), one opacity per slot (DM2_COMPOSITE_ALPHA_PER_SLOT), or (F), one
 * per face, gathered as alpha[render_layers[s]] (DM2_COMPOSITE_ALPHA_PER_FACE); render_layers (B,H,W,L) int32, or NULL with a
 * per-slot alpha (no slot is empty then); background (C) float32 or NULL (no background term).  A slot is empty when its id is
 * negative or, with a per-face alpha, outside [0, F).  Per pixel, all fp32, separate multiplies and adds in the written order,
 * without contraction (bit-exact), from T = 1, O_c = 0, n = 0, for l = 0 .. L-1:
 *   skip an empty slot (neither its values nor its alpha take part: NaNs there are harmless);
 *   a = the slot's alpha as it stands (no clamp; a non-finite a of a non-empty slot propagates);
 *   w = a * T;   O_c = O_c + values[l,c] * w for every c (also when w == 0);   T = T * (1 - a);   n = l + 1;
 *   stop once T < 1e-4 (the slots behind take no part).
 * out[c] = O_c + T * background[c] (O_c without a background) (B,H,W,C); out_acc = 1 - T (B,H,W); out_final_T = T (B,H,W);
 * out_n_contrib = n (B,H,W) int32: what the backward takes.  out_acc, out_final_T and out_n_contrib may each be NULL.  Every
 * element of the outputs is written: no pre-fill.  L == 0: out = background (or 0), T = 1, n = 0; values and alpha may then be
 * NULL. */
#define DM2_COMPOSITE_ALPHA_PER_SLOT 0
#define DM2_COMPOSITE_ALPHA_PER_FACE 1
int dm2_composite(int32_t B, int32_t H, int32_t W, int32_t L, int32_t C, int32_t F, int32_t alpha_mode, const float* values,
                  const float* alpha, const int32_t* render_layers, const float* background, float* out, float* out_acc,
                  float* out_final_T, int32_t* out_n_contrib, void* stream);
/* Gradients of dm2_composite for upstream g = dL_dout (B,H,W,C) and gA = dL_dacc (B,H,W); either may be NULL (zero; both NULL:
 * nothing runs and nothing is written).  n_contrib (B,H,W) is the forward's: slot l of a pixel blended when it is not empty and
 * l < n_contrib.  Per pixel, over its blended slots in order, T_l the transmittance in front of slot l (no division anywhere:
 * an alpha of exactly 1 is fine):
 *   dL_dvalues[l,c] = (a_l * T_l) * g[c];
 *   S_l = sum_c g[c] * values[l,c];   K = sum_c g[c] * background[c] - gA   (missing terms 0);
 *   from the last blended slot backwards, starting at R = K:   dL/da_l = T_l * (S_l - R),   then R = a_l * S_l + (1 - a_l) * R.
 * dL_dvalues (B,H,W,L,C): every element is written, zeros in empty slots and behind the stop.  dL_dalpha per slot (B,H,W,L):
 * likewise, a pure function of the inputs.  dL_dalpha per face (F): dL/da_l is added to dL_dalpha[render_layers[s]] over
 * views, pixels and slots; zero-filled by the caller; float atomics: its last bits may vary from run to run.  Either output
 * pointer may be NULL (not wanted: no phase of the kernel runs for it).  background gets no gradient. */
int dm2_composite_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t C, int32_t F, int32_t alpha_mode,
                           const float* values, const float* alpha, const int32_t* render_layers, const float* background,
                           const int32_t* n_contrib, const float* dL_dout, const float* dL_dacc, float* dL_dvalues,
                           float* dL_dalpha, void* stream);

/* Renderer.coverage: the analytic pixel coverage of every listed slot, the factor that makes a face's opacity an anti-aliased
 * alpha on the deferred path (alpha = faces_opacity[id] * cov into dm2_composite) and lets a silhouette loss reach the vertices.
 * render_layers (B,H,W,L) int32 face ids over the full frame; verts_image (B,P,2) float32, the projected vertices in pixel
 * units; faces (F,3) int32; 0 <= temperature <= 1.  Per slot (b, y, x, l) with id f, all fp32, without contraction:
 *   empty slot (f outside [0, F), or faces[f] names a vertex outside [0, P)): cov = 0;
 *   temperature == 0: cov = 1 in every other slot (no clip is evaluated);
 *   otherwise the triangle verts_image[b, faces[f]] is CCW-reordered and its six AA tables are built as under
 *   DM2_FLAG_TABLES_FROM_IMAGE; area = its overlap with the pixel [x, x+1] x [y, y+1] by the reference's clipper (aa.h:446-504);
 *   a clipper error or area == 0: cov = 0 (dm2_forward skips such a face); else
 *   cov = (float)(1.0 * (double)(1.0f - temperature) + (double)(area * temperature))   (forward.cu:375-378 for a hit).
 * Whether the pixel's ray hits the face is not looked at.  Every element of out_cov (B,H,W,L) is written: no pre-fill.
 * win (NULL: the full frame): render_layers and out_cov are (B,H,W,L) of the window, and the pixel of slot (b, y, x, l) is
 * [x + pmx, x + pmx + 1] x [y + pmy, y + pmy + 1] with (pmx, pmy) = patch_min[b]; verts_image stays in frame units.  Per-pixel:
 * the result is the crop of the full-frame call on layers embedded in a frame of -1.  Only win->patch_min is read (full_W,
 * full_H are not needed).
 * inside (NULL: every slot as above): the inside bytes (B,H,W,L) of dm2_rasterize_run with overlap != 0.  A non-empty slot with
 * inside == 0 mixes as a face that only grazes the pixel (forward.cu:379-381):
 * cov = (float)(0.0 * (double)(1.0f - temperature) + (double)(area * temperature)) = area * temperature, and cov = 0 at
 * temperature 0; a slot with inside != 0 is as above.  The gradient is dm2_coverage_backward's either way (dL_dcov * temperature
 * * d(area)/d(corner)): the mask is not needed there. */
int dm2_coverage(int32_t B, int32_t H, int32_t W, int32_t L, int32_t P, int32_t F, float temperature, const dm2_window* win,
                 const int32_t* render_layers, const uint8_t* inside, const float* verts_image, const int32_t* faces,
                 float* out_cov, void* stream);
/* Gradient of dm2_coverage for upstream dL_dcov (B,H,W,L): every slot with a non-zero cov adds
 * dL_dcov[s] * temperature * d(area)/d(corner k) to dL_dverts_image[b, v] (B,P,2), v the face's vertex that the reorder put at
 * corner k; the Jacobian is the reference clipper's (zero at full cover).  dL_dverts_image is zero-filled by the caller; float
 * atomics: its last bits may vary from run to run.  temperature == 0, dL_dcov NULL or dL_dverts_image NULL: nothing runs.
 * win (NULL: the full frame): as for dm2_coverage; render_layers and dL_dcov are the window's. */
int dm2_coverage_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t P, int32_t F, float temperature,
                          const dm2_window* win, const int32_t* render_layers, const float* verts_image,
                          const int32_t* faces, const float* dL_dcov, float* dL_dverts_image, void* stream);

/* Renderer.vertex_normals: area-weighted smooth vertex normals of a triangle mesh, differentiable w.r.t. the vertices, without
 * float atomics.  verts (P,3) float32, faces (F,3) int32, 3 F < 2^31.  A face is valid when its three ids lie in [0, P).
 * The inverted index (Renderer.vertex_adjacency builds it; a pure function of faces): corners (3F) int32 holds the corner
 * numbers 3 f + k ordered by (vertex id, corner number) ascending, the corners of invalid faces at the end; offsets (P+1) int32:
 * vertex p owns corners[offsets[p] .. offsets[p+1]), offsets[P] = the number of valid corners.  (Offsets are clamped to
 * [0, 3F] and an entry of corners outside [0, 3F) is passed over: an index not built that way cannot address out of bounds.)
 * All fp32, separate multiplies and adds in the written order, without contraction:
 *   face normal (valid faces): e1 = p1 - p0, e2 = p2 - p0, N = e1 x e2 = (e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z,
 *     e1.x * e2.y - e1.y * e2.x), not normalised: it weights by area;
 *   vertex sum: s_p = (((0 + N_c0) + N_c1) + ...) over the vertex's corners in corners' order (N_c = N of face c / 3); a face
 *     that names a vertex twice contributes its (zero) N once per corner; an invalid face contributes to no vertex;
 *   len = sqrtf((s.x * s.x + s.y * s.y) + s.z * s.z);
 *   normalize != 0: out = s / len per component where len > 0 and finite, zeros elsewhere (isolated vertices, exact
 *     cancellation, overflow, NaN); normalize == 0: out = s.
 * Every element of out_normals (P,3) and, when not NULL, out_len (P) = len is written (the backward takes both).  scratch:
 * dm2_vertex_normals_scratch_bytes(P, F, 0) = 16 F bytes, 16-byte aligned, of this call only (the face normals in 16-byte rows).
 * The gradient (faces and the index are constants), for upstream g = dL_dnormals (P,3):
 *   d_p = (g_p - n_p (n_p . g_p)) / len_p where the forward's len (the argument len) is > 0 and finite, else zeros;
 *     normalize == 0: d_p = g_p.  n_p and len_p of this line are not the forward's fp32 values: the backward evaluates edges,
 *     cross products, the vertex sum (in corners' order) and the length again in double and rounds d_p to fp32, because the
 *     fp32 normal of a face whose edges meet at a small angle a is good to u / sin(a) only and d would inherit that error
 *     whole.  The arguments normals and len stand in where the double sum has no direction although len says there is one;
 *   per valid face (fp32 again): D = (d_v0 + d_v1) + d_v2, c1 = e2 x D, c2 = D x e1, c0 = -(c1 + c2);
 *   dL_dverts[p] = (((0 + c_k0) + c_k1) + ...) over its corners in corners' order; every element of dL_dverts (P,3) is written.
 * scratch: dm2_vertex_normals_scratch_bytes(P, F, 1) = 16 (P + 3 F) bytes (d, then the corner terms; the double face normals,
 * 32 F bytes, use the corner terms' place before those are written).  No float atomics either
 * way: two calls with the same inputs give the same bits.  dL_dnormals or dL_dverts NULL: nothing runs.  normals / len may be
 * NULL when normalize == 0. */
size_t dm2_vertex_normals_scratch_bytes(int32_t P, int32_t F, int32_t backward);
int dm2_vertex_normals(int32_t P, int32_t F, int32_t normalize, const float* verts, const int32_t* faces, const int32_t* offsets,
                       const int32_t* corners, void* scratch, size_t scratch_bytes, float* out_normals, float* out_len, void* stream);
int dm2_vertex_normals_backward(int32_t P, int32_t F, int32_t normalize, const float* verts, const int32_t* faces,
                                const int32_t* offsets, const int32_t* corners, const float* normals, const float* len,
                                const float* dL_dnormals, void* scratch, size_t scratch_bytes, float* dL_dverts, void* stream);

/* Renderer.shading_vectors: per slot s = (b, y, x, l) the vectors a shader needs, from dm2_rasterize_run's t, the pixel's own
 * ray and (optionally) dm2_interpolate's normal.  render_layers (B,H,W,L) int32, t (B,H,W,L) float32, normals (B,H,W,L,3)
 * float32 of any length or NULL.  The ray (ro, rd) of the slot's pixel is the one the rasterizer used: image_ray_o / image_ray_d
 * (B,H,W,3), or with flags = DM2_FLAG_ANALYTIC_RAYS the ray computed from ray_cam (B,32) (dm2_render_desc) for a W x H image.
 * win: the arrays are a window's (dm2_window: the ray tensors the window's own cut, the analytic ray that of frame pixel
 * (x + patch_min[b][0], y + patch_min[b][1]) in full_W x full_H); NULL: the full frame.  All fp32 in the written order,
 * without contraction:
 *   empty slot (id < 0, or t not finite): every output is zero and no gradient flows;
 *   position = ro + t * rd per component (one multiply, one add);   view = -rd;
 *   nl = sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z); where nl is not finite (a component that is not finite makes it so) or
 *     nl == 0: normal = reflection = 0 and normals gets no gradient (position and view are written all the same); otherwise
 *   normal = n / nl;   c = (normal.x * view.x + normal.y * view.y) + normal.z * view.z;
 *   reflection = (2.0f * c) * normal - view   (the same bits for n and -n).
 * out_position, out_view and, with normals, out_normal, out_reflection, each (B,H,W,L,3): every element is written.
 * Gradients, for upstream g_position, g_normal, g_reflection (each (B,H,W,L,3) or NULL = zero; view has none):
 *   dL_dt[s] = (g_position.x * rd.x + g_position.y * rd.y) + g_position.z * rd.z;
 *   G = g_normal + 2 c g_reflection + 2 (g_reflection . normal) view,  dL_dnormals[s] = (G - normal (normal . G)) / nl:
 *   orthogonal to n.  Nothing flows to the cameras or through the rays.  dL_dt (B,H,W,L) / dL_dnormals (B,H,W,L,3): NULL = not
 *   wanted; every element of the others is written, zeros in empty slots; no atomics.  Both NULL: nothing runs. */
int dm2_shading_vectors_window(int32_t B, int32_t H, int32_t W, int32_t L, int32_t flags, const dm2_window* win,
                               const int32_t* render_layers, const float* t, const float* normals, const float* image_ray_o,
                               const float* image_ray_d, const float* ray_cam, float* out_position, float* out_view, float* out_normal,
                               float* out_reflection, void* stream);
int dm2_shading_vectors_backward_window(int32_t B, int32_t H, int32_t W, int32_t L, int32_t flags, const dm2_window* win,
                                        const int32_t* render_layers, const float* t, const float* normals, const float* image_ray_o,
                                        const float* image_ray_d, const float* ray_cam, const float* g_position, const float* g_normal,
                                        const float* g_reflection, float* dL_dt, float* dL_dnormals, void* stream);

/* Differentiable compositing of caller-supplied face layers (LayeredRenderer.render).
 * Per pixel of view b, with T = 1, C = D = 0, for l = 0..L-1 and f = render_layers[b,y,x,l]:
 *   1. skip f < 0 or f >= F (holes and out-of-range ids are allowed and never read through);
 *   2. intersect the pixel's ray (image_ray_o / image_ray_d, or DM2_FLAG_ANALYTIC_RAYS) with verts[faces[f]]
 *      (Moeller-Trumbore as the Renderer's kernels evaluate it); skip an edge case (zero denominator);
 *   3. clamp the barycentrics; skip unless the clamp code is 0 (Renderer's coverage at aa_temperature 0);
 *   4. i0 = 1-u-v, i1 = u, i2 = v; iC = (i0 c0 + i1 c1 + i2 c2) * faces_intense[b,f]; iD = i0 z0 + i1 z1 + i2 z2 with
 *      z = verts_ndc[b,.,2]; alpha = faces_opacity[f];
 *   5. C += iC alpha T, D += iD alpha T, T *= 1 - alpha; stop once T < 1e-4.
 * out_color = C + T background (B,H,W,3), out_depth = D + T (B,H,W; NDC depth, background 1), out_final_T = T (B,H,W),
 * out_n_contrib (B,H,W) int32 = 1 + the index of the last layer that blended (0: none).  out_final_T may be NULL;
 * out_n_contrib is what the backward takes.  Bit-exact: the same fp32 operations, in the same order, as the
 * point-sampled Renderer forward.
 * win (NULL: the full frame): d->W, d->H and every (B,H,W,...) array are the window's; a window pixel's ray is its frame
 * pixel's (the window's cut of the ray tensors, or DM2_FLAG_ANALYTIC_RAYS at the absolute pixel with full_W, full_H -- the only
 * place the origin is used).  Per-pixel: the crop of the full-frame call on layers embedded in a frame of -1.
 * out_face_weights (B,F) float32 or NULL (not wanted: the kernel without that work runs), zero-filled by the caller; every
 * blend adds alpha * T (faces_opacity[f] times the transmittance in front of the layer) to out_face_weights[b * F + f] -- a
 * face listed twice in one pixel's layers counts twice.  Float atomics. */
typedef struct dm2_layer_composite_desc {
    int32_t B, P, F;
    int32_t W, H, L;              /* full frame (with a dm2_window: the window's) width/height, layers per pixel */
    int32_t flags;                /* DM2_FLAG_ANALYTIC_RAYS */
    const int32_t* render_layers; /* (B,H,W,L) */
    const float* verts;           /* (P,3) */
    const int32_t* faces;         /* (F,3) */
    const float* verts_color;     /* (P,3) */
    const float* faces_opacity;   /* (F) */
    const float* faces_intense;   /* (B,F) */
    const float* verts_ndc;       /* (B,P,3) */
    const float* background;      /* (3) */
    const float* image_ray_o;     /* (B,H,W,3); may be NULL with DM2_FLAG_ANALYTIC_RAYS */
    const float* image_ray_d;     /* (B,H,W,3); may be NULL with DM2_FLAG_ANALYTIC_RAYS */
    const float* ray_cam;         /* DM2_FLAG_ANALYTIC_RAYS: (B,32), see dm2_render_desc */
} dm2_layer_composite_desc;

int dm2_layers_composite(const dm2_layer_composite_desc* d, const dm2_window* win, float* out_color, float* out_depth,
                         float* out_final_T, int32_t* out_n_contrib, float* out_face_weights, void* stream);
/* Gradients of the composite w.r.t. verts_color (P,3), faces_opacity (F), verts_ndc (B,P,3; only z written) and
 * faces_intense (B,F); the four outputs must be zero-filled by the caller.  No gradient reaches verts through the
 * barycentrics (the layers are piecewise constant in the points) and none reaches background.  n_contrib: what the
 * forward of the same inputs wrote.  Division-free in alpha: opacities of exactly 1.0 are fine.  win (NULL: the full frame):
 * the forward's.  dL_dout_alpha (B,H,W) or NULL (zero: the kernel without that term runs): the upstream gradient of
 * alpha = 1 - out_final_T; it reaches dL_dfaces_opacity only. */
int dm2_layers_composite_backward(const dm2_layer_composite_desc* d, const dm2_window* win, const float* dL_dout_color,
                                  const float* dL_dout_depth, const float* dL_dout_alpha,
                                  const int32_t* n_contrib, float* dL_dverts_color, float* dL_dfaces_opacity,
                                  float* dL_dverts_ndc, float* dL_dfaces_intense, void* stream);

/* Host prep of Renderer.forward / LayeredRenderer.generate, fused.
 * Replaces the ~20 torch kernels of the reference's Python host layer:
 *   compute_verts_ndc_image  dmesh2_renderer/__init__.py:239-262  (projection, |w| clamp, NDC -> image)
 *   Triangles                dmesh2_renderer/pyrenderer.py:6-30   (CCW reorder + the six AA tables)
 * mv / proj are the (B,4,4) matrices of the selected cameras, row-major, applied as
 * `hom @ mv^T @ proj^T`.  Any of the eight outputs may be NULL (LayeredRenderer needs the
 * first two only); with F == 0 or all aa_* NULL only the projection runs. */
typedef struct dm2_prep_desc {
    int32_t B, P, F;
    int32_t W, H;                 /* FULL image width / height (Renderer.width/height), not the patch */
    const float* verts;           /* (P,3) */
    const int32_t* faces;         /* (F,3) */
    const float* mv;              /* (B,4,4) */
    const float* proj;            /* (B,4,4) */
    float* verts_ndc;             /* (B,P,3) out */
    float* verts_image;           /* (B,P,2) out (input of the backward when non-NULL there) */
    float* aa_face_verts;         /* (B,F,3,2) out */
    float* aa_face_edges;         /* (B,F,3,2) out */
    uint8_t* aa_face_edges_iszero;/* (B,F,3,2) out, bool */
    float* aa_face_edges_recip;   /* (B,F,3,2) out */
    float* aa_face_edges_normal;  /* (B,F,3,2) out */
    float* aa_face_edges_normal_c;/* (B,F,3) out */
} dm2_prep_desc;

int dm2_prepare_faces(const dm2_prep_desc* d, void* stream);
/* The gradient torch autograd sends back through the host prep: upstream gradients of verts_ndc
 * (B,P,3), verts_image (B,P,2) and aa_face_verts (B,F,3,2) (each may be NULL) -> g_verts (P,3),
 * overwritten.  image_grad_scratch: B*P*2 floats of caller scratch.  Only the input fields of `d`
 * are read. */
int dm2_prepare_faces_backward(const dm2_prep_desc* d, const float* g_verts_ndc, const float* g_verts_image,
                               const float* g_aa_face_verts, float* image_grad_scratch, float* g_verts,
                               void* stream);
/* dm2_prepare_faces_backward that can also return the gradients of the camera matrices: g_mv and g_proj (B,4,4) row-major,
 * overwritten, of the projection `hom @ mv^T @ proj^T` -> |w| clamp -> NDC -> image units, i.e. per view b
 *   g_proj[b][j][k] = sum_p gc_j t_k,   g_mv[b][j][k] = sum_p gt_j hom_k,
 * with hom = (x, y, z, 1), t = mv_b . hom, gc the gradient of the clip point (gc[3] = 0 where the clamp fired) and
 * gt = proj_b^T . gc.  g_verts, g_mv and g_proj may each be NULL (NULL g_verts: d(verts) is not computed; P = 0 or no
 * upstream gradient: zeros).  camera_scratch: dm2_prepare_faces_camera_scratch_bytes(B, P) bytes of caller scratch
 * (= B * min(ceil(P / 256), 1024) * 256), read only when g_mv or g_proj is non-NULL.  No float atomics on the camera route:
 * two calls with the same inputs give the same bits (the aa_face_verts route feeds it through the per-vertex scatter of
 * image_grad_scratch, whose float atomics add a vertex's corners in no fixed order).  With g_mv = g_proj = NULL this is
 * dm2_prepare_faces_backward, to the bit. */
size_t dm2_prepare_faces_camera_scratch_bytes(int32_t B, int32_t P);
int dm2_prepare_faces_backward_camera(const dm2_prep_desc* d, const float* g_verts_ndc, const float* g_verts_image,
                                      const float* g_aa_face_verts, float* image_grad_scratch, float* g_verts, float* g_mv,
                                      float* g_proj, void* camera_scratch, void* stream);

/* Device side of the sparse leaf-gradient exchange of a frame sharded by tile rows over N ranks (the
 * collectives themselves belong to the caller: dmesh2_renderer_amd/sharding.py drives torch.distributed / RCCL).  Rows are
 * owned by contiguous id ranges: face f by rank f / ceil(F/N), vertex v by rank v / ceil(P/N).
 *   dm2_exchange_mark    after dm2_forward / dm2_forward_run: flags (P + F bytes of caller scratch: F face flags, then P vertex flags) mark the
 *                        faces this rank's tile lists hold (any view) and their vertices; counts (2 N uint32, device):
 *                        [2 o] faces / [2 o + 1] vertices flagged in owner o's range = the rows this rank will send to o.
 *   dm2_exchange_pack    after the backward: the send buffer, per owner o [counts[2 o] rows of (2 + B) floats: id bits, dopacity,
 *                        dintense(b = 0..B-1) | counts[2 o + 1] rows of 7 floats: id bits, dverts(3), dverts_color(3)];
 *                        cursors: 2 N uint32 of scratch.  Rows of one segment in no particular order.
 *   dm2_exchange_unpack  owner `rank`: recv holds, per source s, [recv_counts[2 s] face rows | recv_counts[2 s + 1] vertex rows]
 *                        (`rows` rows in all; recv_counts is a HOST array -- the caller needed these numbers on the host for the
 *                        all-to-all anyway); they are summed, source by source, into slice_v (ceil(P/N), 6) and slice_f
 *                        (ceil(F/N), 1 + B), which the call zero-fills first. */
int dm2_exchange_mark(int32_t B, int32_t P, int32_t F, int32_t N, const int32_t* faces, const void* face_scratch, size_t face_bytes,
                      uint8_t* flags, uint32_t* counts, void* stream);
int dm2_exchange_pack(int32_t B, int32_t P, int32_t F, int32_t N, const uint8_t* flags, const uint32_t* counts, uint32_t* cursors,
                      const float* dverts, const float* dverts_color, const float* dfaces_opacity, const float* dfaces_intense,
                      float* send, void* stream);
int dm2_exchange_unpack(int32_t B, int32_t P, int32_t F, int32_t N, int32_t rank, const float* recv, const uint32_t* recv_counts,
                        int64_t rows, float* slice_v, float* slice_f, void* stream);

/* Introspection for tests/bench: copy pieces of the scratch state to caller
 * (device) buffers.  what: 0 ranges (B*tiles*2 u32, from image scratch),
 * 1 face_list (num_rendered u32, from binning scratch), 2 final_T, 3 final_prev_T
 * (N f32), 4 n_contrib (N u32), 5 first_face, 6 first_tet (N i32, layer image scratch),
 * 8 tiles_touched (count = B*F u32, from face scratch; aux = the aux of dm2_scratch_bytes),
 * 9 hit_valid (4 u32 from binning scratch: [0] what the forward left, [1] pair-pool slots it claimed, [2] tie-queue entries),
 * 10 hit_valid, all 8 u32: behind the four of item 9, [4] the tie-queue length the last tie pass saw and [5] how many of those
 * entries the backward wrote straight to the queue, round its per-block buffer (the destination of item 9 holds 4 words only). */
int dm2_debug_fetch(int what, int64_t count, int64_t aux, int64_t num_rendered,
                    const void* scratch, size_t scratch_bytes, void* dst, void* stream);

/* Test hook: run one of the device clippers on n independent (triangle, pixel) pairs.  Tables as the reference's
 * Triangles builds them (pyrenderer.py:6-30), n x the per-face layout of dm2_render_desc; pixmin (n,2) float: the
 * pixel's (x, y) origin, unit size.  variant 0: the generic clipper of the per-pixel-walk kernels, area + Jacobian in
 * the reference's order (aa.h:151-504); 1: the forward's area-only clipper; 2: the forward's accept / reject decision,
 * then the backward's segment formulation of area + Jacobian; 3: the same with the reference's fan sum over its corners
 * (the area bit-identical to the forward's, what the exact-clipper backward uses for faces with opacity > 0.9); 4: the
 * default backward's Jacobian without a polygon (code -1 and a zero Jacobian: the pair is a tie and takes variant 2's
 * route; area: the forward's).  Outputs: area (n), grad (n,3,2), code (n) int32 --
 * 0 = no error, non-zero = the reference reports one of its errors E00..E05 (dmesh2_renderer/README.md; the
 * composite kernels only ever test != 0); area and grad are zero where code != 0. */
int dm2_debug_aa_overlap(int variant, int64_t n, const float* aa_face_verts, const float* aa_face_edges,
                         const uint8_t* aa_face_edges_iszero, const float* aa_face_edges_recip,
                         const float* aa_face_edges_normal, const float* aa_face_edges_normal_c,
                         const float* pixmin, float* area, float* grad, int32_t* code, void* stream);

/* Optional per-stage timing (bench/profiling only; off by default).  When enabled, the
 * forward/backward/layers entry points record hipEvents on `stream` around every stage of
 * the calling thread's next calls; dm2_profile_read waits for the last one and returns the
 * milliseconds of each stage of the most recent forward_plan/forward_run/backward call:
 * [0] preprocess + tile scan  [1] scatter into the tile segments (radix route: scan + key emit)
 * [2] per-tile sorts (radix route: the radix sort)  [3] tile ranges (radix route only)
 * [4] forward composite [5] backward composite [6] the backward's tie pass (k_aa_ties; 0 when another backward kernel
 * ran).  Returns the number of values written. */
#define DM2_PROFILE_STAGES 7
void dm2_profile_enable(int on);
int dm2_profile_read(float* ms, int capacity);

/* Diagnostic builds only (-DDM2_STAMPS): copy the in-kernel cycle-stamp table (2 kernels x 16
 * segments, shader cycles summed over waves) to the HOST array `out`; returns the number of
 * values, or -1 in a product build (which contains no stamps). */
int dm2_debug_stamps(uint64_t* out, int capacity, int reset);

#ifdef __cplusplus
}
#endif
#endif /* DM2_HIP_H */
