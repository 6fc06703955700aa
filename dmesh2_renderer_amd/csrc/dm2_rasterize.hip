// dm2_rasterize.hip -- Renderer.rasterize: the L nearest hits of every pixel's ray on a triangle mesh (no tetrahedra):
//   k_rasterize<KR>   per pixel the first L faces its ray hits in (t, face id) order, with barycentrics and t
//   k_rasterize_bwd   d(bary, t)/d(verts) of the listed hits
//   k_rasterize_overlap<KR>, k_rasterize_overlap_bwd   the overlap mode (below): the faces that overlap the pixel's square
//
// Contract (include/dm2_hip.h, dm2_rasterize_run): per pixel of view b the candidates are the faces of its tile's list
// (dm2_layers_plan: the verts_image bbox touches the tile, the NDC depth cull keeps the face) whose face_existence is not 0;
// a hit is ray_tri_intersection with t >= 0, u >= 0, v >= 0, u + v <= 1 (k_first_intersect's test) on a face whose plane the
// ray does not lie in (rz_off_plane, below); the hits are ordered by ascending (t, face id) and the first L are listed with
// bary = (1 - u - v, u, v) and t.  -ffp-contract=off: bit-exact.
//
// Window (dm2_window): d.W, d.H, the tile grid, the tile lists and every (B,H,W,...) array are the window's; only the ray knows
// the frame: pixel_ray gets the absolute pixel (px + origin) and the frame's size.  A null origin is (0, 0) in d.W x d.H.
//
// Layout: one lane per pixel, 16 x 16 tiles, the view on blockIdx.z; list chunks staged in LDS as k_first_intersect stages
// them, the existence filter applied (and the survivors compacted) while staging.  Each lane keeps its KR nearest hits so far
// in registers, sorted; a new hit goes in by a fully unrolled compare-and-swap over the slots (static indices only: no
// scratch).  KR = the smallest of 1, 2, 4, 8, 16 that holds L; L > 16 runs in passes of 16, each keeping only hits strictly
// after the previous pass's last (t, id) -- carried in registers from pass to pass.
//
// Early exit (not part of the result): the tile list is sorted by min depth, so once a lane holds its slots full, a face
// whose min depth lies beyond the largest max depth of the held faces cannot come nearer along this ray and the lane stops
// (the K-wide form of k_first_intersect's stop, forward.cu:648-651).  Depth along a ray grows with t in front of the camera;
// a face that crosses the camera plane has no such bound, as in the first-hit pass of generate (and the plan may not have
// put it into the tile's list at all: its bbox is that of mirrored projections).  The stop relies on a held hit's t lying
// in its face's depth range: rz_off_plane keeps the noise t of a ray in the face's plane out of the slots.
//
// Overlap mode (include/dm2_hip.h, dm2_rasterize_run with overlap != 0): the same candidates; a candidate is listed iff (a) its
// projected triangle verts_image[b, faces[f]] overlaps the pixel's square [X, X+1] x [Y, Y+1] (frame coordinates) -- the tables
// of cov_tables_pts, tri_pix_overlap_area_only without error and with area != 0: k_coverage's clip, bit for bit, so coverage of
// a listed slot is never 0 by the "misses the pixel" rule -- (b) ray_tri_intersection succeeds and rz_off_plane holds, and (c)
// the slot's t >= 0.  With (uc, vc, code) = clamp_bary_uv(u, v): bary = (1 - uc - vc, uc, vc), inside = (code == 0), and
// t = tuv.x for code 0, else rz_proj_t: the ray parameter of the clamped point's projection onto the ray (continuous across the
// triangle's edge: on it the clamped point is the hit).  Order (t, id), the first L, passes of 16 as above.
// Staging: per kept face the record holds, next to the three vertices, the three image corners and their bbox; a lane first
// rejects by that bbox against its pixel square (the clipper's own first test, aa.h:96-101, so the reject changes nothing) and
// only survivors pay for the ray test, the tables and the clip.
// Early exit: NONE.  An off-triangle slot's t is not a point of the pixel's ray on the face, so "t lies in the face's depth
// range", which the standard mode's stop rests on, is not known to hold for a held slot; no other bound is proved here, and
// the walk is exhaustive (a pass ends early only when every lane of the block has run out of faces in an earlier pass).
//
// Backward: per listed slot the ray is intersected again and dL/dp_k = (g1 - g0) du/dp_k + (g2 - g0) dv/dp_k + g_t dt/dp_k,
// in fp64 (rz_hit_grad), added into the block's FaceTable (dm2_face_table.h; fp64 accumulators), flushed as fp32 atomics.
#include <hip/hip_runtime.h>

#include "dm2_clip_area.h"
#include "dm2_cov_tables.h"
#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_stage.h"
#include "dm2_state.h"

namespace dm2 {

constexpr int RZ_CHUNK = TILE_PIX;  // list entries staged per round: one per lane
constexpr int RZ_PASS = 16;         // the longest register list; L > 16 runs in passes of 16
constexpr int RZ_NCOMP = 9;         // d verts: 3 vertices x 3 coordinates
constexpr int RZ_NO_ID = 0x7FFFFFFF;

struct __attribute__((aligned(16))) RzRec {
    float v[9];
    float min_d, max_d;
    int face_id;
};
static_assert(sizeof(RzRec) == 48, "RzRec");

// a lane's nearest hits so far, ascending (t, id); empty slots hold t = +inf, id = RZ_NO_ID, md = -inf
template <int KR>
struct RzList {
    float t[KR], u[KR], v[KR], md[KR];
    int id[KR];
};

// The hit rule's second half: the ray is off the face's plane, cos^2(rd, n) > RZ_PLANE_COS2 (|cos| > 5e-4) for n = E1 x E2.
// For a ray in the plane Moeller-Trumbore's denom = -(rd . n) is rounding noise, seldom exactly 0, and t, u, v are noise that
// can pass the inside test at any t ("phantom hits": listed nearest, with a gradient divided by rd . n ~ 0).  Above the bound
// denom holds its value to ~1e-7 / 5e-4 of itself.  A zero-area face (n == 0 exactly for a repeated vertex) never passes.
// Evaluated for the few candidates that pass the inside test only.  fp32, this order, uncontracted (rasterize_ref.off_plane32).
constexpr float RZ_PLANE_COS2 = 2.5e-7f;
__device__ __forceinline__ bool rz_off_plane(f3 rd, f3 p0, f3 p1, f3 p2) {
    const f3 n = cross(p1 - p0, p2 - p0);
    const float dn = dot(rd, n);
    return dn * dn > (RZ_PLANE_COS2 * dot(n, n)) * dot(rd, rd);
}

__device__ __forceinline__ bool rz_before(float ta, int ia, float tb, int ib) { return ta < tb || (ta == tb && ia < ib); }

// insert a hit into the first Lp slots (the one pushed out of slot Lp - 1 is dropped); slots Lp.. stay empty
template <int KR>
__device__ __forceinline__ void rz_insert(RzList<KR>& h, int Lp, float t, int id, float u, float v, float md) {
#pragma unroll
    for (int k = 0; k < KR; k++) {
        const bool sw = k < Lp && rz_before(t, id, h.t[k], h.id[k]);
        const float t0 = h.t[k], u0 = h.u[k], v0 = h.v[k], m0 = h.md[k];
        const int i0 = h.id[k];
        h.t[k] = sw ? t : t0; h.id[k] = sw ? id : i0; h.u[k] = sw ? u : u0; h.v[k] = sw ? v : v0; h.md[k] = sw ? md : m0;
        t = sw ? t0 : t; id = sw ? i0 : id; u = sw ? u0 : u; v = sw ? v0 : v; md = sw ? m0 : md;
    }
}

template <int KR>
__global__ void __launch_bounds__(TILE_PIX)
k_rasterize(dm2_layers_desc d, dm2_window win, const float* __restrict__ min_depths, const float* __restrict__ max_depths,
            const uint2* __restrict__ ranges, const uint32_t* __restrict__ face_list, int32_t* __restrict__ out_layers,
            int32_t* __restrict__ out_cnt, float* __restrict__ out_bary, float* __restrict__ out_t) {
    __shared__ RzRec recs[RZ_CHUNK];
    __shared__ int s_kept[TILE_PIX / 64];
    const int b = blockIdx.z;
    const uint32_t gx = (d.W + TILE - 1) / TILE, gy = (d.H + TILE - 1) / TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto [px, py, inside, pix] = tile_pixel(tid, d.W, d.H);
    f3 ro = {0, 0, 0}, rd = {0, 0, 0};
    const WinOrigin org = window_origin(win.patch_min);
    if (inside) pixel_ray(d, b, pix, px + org.x, py + org.y, win.full_W, win.full_H, ro, rd);
    const uint32_t tile = ((uint32_t)b * gy + blockIdx.y) * gx + blockIdx.x;
    const uint2 range = ranges[tile];
    const int total = (int)(range.y - range.x);
    const int L = d.L;
    const int npass = KR < RZ_PASS ? 1 : (L + RZ_PASS - 1) / RZ_PASS;
    bool exhausted = !inside;                 // no hit left behind the previous pass's last
    float prev_t = 0.0f;
    int prev_id = -1, listed = 0;
    for (int pass = 0; pass < npass; pass++) {
        const int Lp = min(KR, L - pass * RZ_PASS);
        RzList<KR> h;
#pragma unroll
        for (int k = 0; k < KR; k++) { h.t[k] = __builtin_inff(); h.id[k] = RZ_NO_ID; h.u[k] = 0.f; h.v[k] = 0.f; h.md[k] = -__builtin_inff(); }
        int cnt = 0;                          // hits held, <= Lp
        float bound = -__builtin_inff();      // the largest max depth of the held hits, once cnt == Lp
        bool done = exhausted;
        for (int base = 0; base < total; base += RZ_CHUNK) {
            if (__syncthreads_count(done) == TILE_PIX) break;
            const int n = min(RZ_CHUNK, total - base);
            int f = -1;
            bool keep = false;
            if (tid < n) {
                f = (int)face_list[range.x + base + tid];
                keep = !d.face_existence || d.face_existence[f] != 0;
            }
            // the chunk's existing faces, compacted in list order
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_kept[wave] = __popcll(m);
            __syncthreads();
            int before = 0, kept = 0;
#pragma unroll
            for (int w = 0; w < TILE_PIX / 64; w++) {
                const int c = s_kept[w];
                before += w < wave ? c : 0;
                kept += c;
            }
            if (keep) {
                RzRec& r = recs[before + __popcll(m & ((1ull << lane) - 1ull))];
                r.face_id = f;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const int64_t vi = d.faces[3 * (int64_t)f + i];
                    r.v[3 * i] = d.verts[3 * vi]; r.v[3 * i + 1] = d.verts[3 * vi + 1]; r.v[3 * i + 2] = d.verts[3 * vi + 2];
                }
                r.min_d = min_depths[(int64_t)b * d.F + f];
                r.max_d = max_depths[(int64_t)b * d.F + f];
            }
            __syncthreads();
            for (int j = 0; !done && j < kept; j++) {
                const RzRec& r = recs[j];
                if (cnt == Lp && r.min_d > bound) { done = true; break; }
                f3 tuv;
                if (!ray_tri_intersection(ro, rd, {r.v[0], r.v[1], r.v[2]}, {r.v[3], r.v[4], r.v[5]}, {r.v[6], r.v[7], r.v[8]}, tuv)) continue;
                if (!(tuv.x >= 0.0f && tuv.y >= 0.0f && tuv.z >= 0.0f && tuv.y + tuv.z <= 1.0f)) continue;
                if (!rz_off_plane(rd, {r.v[0], r.v[1], r.v[2]}, {r.v[3], r.v[4], r.v[5]}, {r.v[6], r.v[7], r.v[8]})) continue;
                if (pass > 0 && !rz_before(prev_t, prev_id, tuv.x, r.face_id)) continue;    // listed by an earlier pass
                rz_insert<KR>(h, Lp, tuv.x, r.face_id, tuv.y, tuv.z, r.max_d);
                cnt = min(cnt + 1, Lp);
                if (cnt == Lp) {
                    float mx = h.md[0];
#pragma unroll
                    for (int k = 1; k < KR; k++) mx = fmaxf(mx, h.md[k]);
                    bound = mx;
                }
            }
        }
        if (inside) {
            const int64_t o = pix * L + pass * RZ_PASS;
#pragma unroll
            for (int k = 0; k < KR; k++) {
                if (k >= Lp) continue;
                const bool hit = k < cnt;
                out_layers[o + k] = hit ? h.id[k] : -1;
                out_bary[3 * (o + k)] = hit ? 1.0f - h.u[k] - h.v[k] : -1.0f;
                out_bary[3 * (o + k) + 1] = hit ? h.u[k] : -1.0f;
                out_bary[3 * (o + k) + 2] = hit ? h.v[k] : -1.0f;
                out_t[o + k] = hit ? h.t[k] : -1.0f;
            }
        }
        listed += cnt;
        if (cnt < Lp) exhausted = true;       // the walk saw the whole list: nothing is left for a later pass
        prev_t = h.t[KR - 1]; prev_id = h.id[KR - 1];   // (read by a next pass only: then Lp == KR == RZ_PASS and cnt == Lp)
    }
    if (inside) out_cnt[pix] = listed;
}

// ---- overlap mode ---------------------------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) RzORec {
    float bb[4];        // xmin, xmax, ymin, ymax of the image corners (AAFace::bb)
    float v[9];
    int face_id;
    float img[6];       // verts_image of the three vertices, in the face's own order
};
static_assert(sizeof(RzORec) == 80, "RzORec");

// a lane's nearest listed faces so far, ascending (t, id); empty slots hold t = +inf, id = RZ_NO_ID; u, v are the CLAMPED pair
template <int KR>
struct RzOList {
    float t[KR], u[KR], v[KR];
    int id[KR], in[KR];
};

template <int KR>
__device__ __forceinline__ void rz_insert_overlap(RzOList<KR>& h, int Lp, float t, int id, float u, float v, int in) {
#pragma unroll
    for (int k = 0; k < KR; k++) {
        const bool sw = k < Lp && rz_before(t, id, h.t[k], h.id[k]);
        const float t0 = h.t[k], u0 = h.u[k], v0 = h.v[k];
        const int i0 = h.id[k], n0 = h.in[k];
        h.t[k] = sw ? t : t0; h.id[k] = sw ? id : i0; h.u[k] = sw ? u : u0; h.v[k] = sw ? v : v0; h.in[k] = sw ? in : n0;
        t = sw ? t0 : t; id = sw ? i0 : id; u = sw ? u0 : u; v = sw ? v0 : v; in = sw ? n0 : in;
    }
}

// The t of a slot whose clamp code is not 0: the ray parameter of the projection onto the ray of the clamped point
// (1 - uc - vc) p0 + uc p1 + vc p2.  fp32, this order, uncontracted (overlap_ref.proj_t32); dot = (x x + y y) + z z.
__device__ __forceinline__ float rz_proj_t(f3 ro, f3 rd, f3 p0, f3 p1, f3 p2, float uc, float vc) {
    const float b0 = 1.0f - uc - vc;
    const float d0 = dot(p0 - ro, rd), d1 = dot(p1 - ro, rd), d2 = dot(p2 - ro, rd);
    return ((b0 * d0 + uc * d1) + vc * d2) / dot(rd, rd);
}

template <int KR>
__global__ void __launch_bounds__(TILE_PIX)
k_rasterize_overlap(dm2_layers_desc d, dm2_window win, const uint2* __restrict__ ranges, const uint32_t* __restrict__ face_list,
                    int32_t* __restrict__ out_layers, int32_t* __restrict__ out_cnt, float* __restrict__ out_bary,
                    float* __restrict__ out_t, uint8_t* __restrict__ out_inside) {
    __shared__ RzORec recs[RZ_CHUNK];
    __shared__ int s_kept[TILE_PIX / 64];
    const int b = blockIdx.z;
    const uint32_t gx = (d.W + TILE - 1) / TILE, gy = (d.H + TILE - 1) / TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto [px, py, inside, pix] = tile_pixel(tid, d.W, d.H);
    f3 ro = {0, 0, 0}, rd = {0, 0, 0};
    const WinOrigin org = window_origin(win.patch_min);
    if (inside) pixel_ray(d, b, pix, px + org.x, py + org.y, win.full_W, win.full_H, ro, rd);
    // the pixel's square in the frame: verts_image's units (k_coverage's)
    const float pxmin = (float)(px + org.x), pxmax = pxmin + 1, pymin = (float)(py + org.y), pymax = pymin + 1;
    const float2* im = reinterpret_cast<const float2*>(d.verts_image) + (int64_t)b * d.P;
    const uint32_t tile = ((uint32_t)b * gy + blockIdx.y) * gx + blockIdx.x;
    const uint2 range = ranges[tile];
    const int total = (int)(range.y - range.x);
    const int L = d.L;
    const int npass = KR < RZ_PASS ? 1 : (L + RZ_PASS - 1) / RZ_PASS;
    bool exhausted = !inside;                 // nothing left behind the previous pass's last
    float prev_t = 0.0f;
    int prev_id = -1, listed = 0;
    for (int pass = 0; pass < npass; pass++) {
        const int Lp = min(KR, L - pass * RZ_PASS);
        RzOList<KR> h;
#pragma unroll
        for (int k = 0; k < KR; k++) { h.t[k] = __builtin_inff(); h.id[k] = RZ_NO_ID; h.u[k] = 0.f; h.v[k] = 0.f; h.in[k] = 0; }
        int cnt = 0;                          // slots held, <= Lp
        for (int base = 0; base < total; base += RZ_CHUNK) {
            if (__syncthreads_count(exhausted) == TILE_PIX) break;
            const int n = min(RZ_CHUNK, total - base);
            int f = -1;
            bool keep = false;
            if (tid < n) {
                f = (int)face_list[range.x + base + tid];
                keep = !d.face_existence || d.face_existence[f] != 0;
            }
            // the chunk's existing faces, compacted in list order
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_kept[wave] = __popcll(m);
            __syncthreads();
            int before = 0, kept = 0;
#pragma unroll
            for (int w = 0; w < TILE_PIX / 64; w++) {
                const int c = s_kept[w];
                before += w < wave ? c : 0;
                kept += c;
            }
            if (keep) {
                RzORec& r = recs[before + __popcll(m & ((1ull << lane) - 1ull))];
                r.face_id = f;
                float2 q[3];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const int64_t vi = d.faces[3 * (int64_t)f + i];
                    r.v[3 * i] = d.verts[3 * vi]; r.v[3 * i + 1] = d.verts[3 * vi + 1]; r.v[3 * i + 2] = d.verts[3 * vi + 2];
                    q[i] = im[vi];
                    r.img[2 * i] = q[i].x; r.img[2 * i + 1] = q[i].y;
                }
                // AAFace::bb, in cov_tables_pts' order of the (reordered) corners
                const bool flip = cov_flip(q[0], q[1], q[2]);
                const float2 q1 = flip ? q[2] : q[1], q2 = flip ? q[1] : q[2];
                r.bb[0] = fminf(fminf(q[0].x, q1.x), q2.x);
                r.bb[1] = fmaxf(fmaxf(q[0].x, q1.x), q2.x);
                r.bb[2] = fminf(fminf(q[0].y, q1.y), q2.y);
                r.bb[3] = fmaxf(fmaxf(q[0].y, q1.y), q2.y);
            }
            __syncthreads();
            for (int j = 0; !exhausted && j < kept; j++) {
                const RzORec& r = recs[j];
                if ((pxmax < r.bb[0]) || (pxmin > r.bb[1]) || (pymax < r.bb[2]) || (pymin > r.bb[3])) continue;   // aa.h:96-101
                const f3 p0 = {r.v[0], r.v[1], r.v[2]}, p1 = {r.v[3], r.v[4], r.v[5]}, p2 = {r.v[6], r.v[7], r.v[8]};
                f3 tuv;
                if (!ray_tri_intersection(ro, rd, p0, p1, p2, tuv)) continue;
                if (!rz_off_plane(rd, p0, p1, p2)) continue;
                float uc, vc;
                int code;
                clamp_bary_uv(tuv.y, tuv.z, uc, vc, code);
                const float t = code == 0 ? tuv.x : rz_proj_t(ro, rd, p0, p1, p2, uc, vc);
                if (!(t >= 0.0f)) continue;
                if (pass > 0 && !rz_before(prev_t, prev_id, t, r.face_id)) continue;        // listed by an earlier pass
                AAFace a;
                cov_tables_pts(make_float2(r.img[0], r.img[1]), make_float2(r.img[2], r.img[3]), make_float2(r.img[4], r.img[5]), a);
                float area;
                const int err = tri_pix_overlap_area_only(a, pxmin, pxmax, pymin, pymax, 1.0f, area);
                if (err != 0 || area == 0.0f) continue;
                rz_insert_overlap<KR>(h, Lp, t, r.face_id, uc, vc, code == 0 ? 1 : 0);
                cnt = min(cnt + 1, Lp);
            }
        }
        if (inside) {
            const int64_t o = pix * L + pass * RZ_PASS;
#pragma unroll
            for (int k = 0; k < KR; k++) {
                if (k >= Lp) continue;
                const bool hit = k < cnt;
                out_layers[o + k] = hit ? h.id[k] : -1;
                out_bary[3 * (o + k)] = hit ? 1.0f - h.u[k] - h.v[k] : -1.0f;
                out_bary[3 * (o + k) + 1] = hit ? h.u[k] : -1.0f;
                out_bary[3 * (o + k) + 2] = hit ? h.v[k] : -1.0f;
                out_t[o + k] = hit ? h.t[k] : -1.0f;
                out_inside[o + k] = (uint8_t)(hit ? h.in[k] : 0);
            }
        }
        listed += cnt;
        if (cnt < Lp) exhausted = true;       // the walk saw the whole list: nothing is left for a later pass
        prev_t = h.t[KR - 1]; prev_id = h.id[KR - 1];   // (read by a next pass only: then Lp == KR == RZ_PASS and cnt == Lp)
    }
    if (inside) out_cnt[pix] = listed;
}

// One listed hit's gradient, in fp64: with n = E1 x E2, q = n / (rd . n), a = (E2 x n) / |n|^2, b = (n x E1) / |n|^2 (the
// dual basis of E1, E2 in the plane) and the barycentrics w at the hit,
//     dt/dp_k = w_k q,   du/dp_k = -w_k (a - q (rd . a)),   dv/dp_k = -w_k (b - q (rd . b)),
// so dL/dp_k = w_k G with G = -(gu a + gv b) + q (rd . (gu a + gv b) + gt).  The same derivative as ray_tri_intersection_grad
// (du, its corrected dv, and its reference branch's "dv", which is dt); evaluated in fp32 that formula measured 3e-5 of the
// largest entry from float64 on a tet lattice (faces seen at grazing angles), hence fp64 here.  false: rd . n == 0.
// S: float (k_rasterize_bwd) or double (k_rasterize_overlap_bwd, whose gu, gv come through the clamp's chain in fp64).
template <typename S>
__device__ __forceinline__ bool rz_hit_grad(f3 ro_f, f3 rd_f, const float* pa, const float* pb, const float* pc, S gu, S gv,
                                            S gt, double w[3], double G[3]) {
    const double ro[3] = {ro_f.x, ro_f.y, ro_f.z}, rd[3] = {rd_f.x, rd_f.y, rd_f.z};
    const double p0[3] = {pa[0], pa[1], pa[2]};
    double e1[3], e2[3], T[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { e1[i] = (double)pb[i] - p0[i]; e2[i] = (double)pc[i] - p0[i]; T[i] = ro[i] - p0[i]; }
    auto cross = [](const double* x, const double* y, double* o) {
        o[0] = x[1] * y[2] - x[2] * y[1]; o[1] = x[2] * y[0] - x[0] * y[2]; o[2] = x[0] * y[1] - x[1] * y[0];
    };
    auto dot = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
    double n[3], a[3], b[3], X[3];
    cross(e1, e2, n);
    const double dn = dot(rd, n), nn = dot(n, n);
    if (dn == 0.0 || nn == 0.0) return false;
    const double t = -dot(T, n) / dn;
#pragma unroll
    for (int i = 0; i < 3; i++) X[i] = T[i] + t * rd[i];             // the hit relative to p0
    cross(e2, n, a); cross(n, e1, b);
#pragma unroll
    for (int i = 0; i < 3; i++) { a[i] /= nn; b[i] /= nn; }
    const double u = dot(X, a), v = dot(X, b);
    w[0] = 1.0 - u - v; w[1] = u; w[2] = v;
    double s[3];
#pragma unroll
    for (int i = 0; i < 3; i++) s[i] = (double)gu * a[i] + (double)gv * b[i];
    const double k = (dot(rd, s) + (double)gt) / dn;
#pragma unroll
    for (int i = 0; i < 3; i++) G[i] = k * n[i] - s[i];
    return true;
}

__global__ void __launch_bounds__(TILE_PIX)
k_rasterize_bwd(dm2_layers_desc d, dm2_window win, const int32_t* __restrict__ layers, const float* __restrict__ dL_dbary,
                const float* __restrict__ dL_dt, float* __restrict__ dL_dverts) {
    __shared__ FaceTable<double, RZ_NCOMP> tab;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    tab.clear(tid);
    __syncthreads();

    const auto [px, py, inside, pix] = tile_pixel(tid, d.W, d.H);
    const WinOrigin org = window_origin(win.patch_min);
    if (inside) {
        f3 ro, rd;
        pixel_ray(d, b, pix, px + org.x, py + org.y, win.full_W, win.full_H, ro, rd);
        for (int l = 0; l < d.L; l++) {
            const int64_t s = pix * d.L + l;
            const int f = layers[s];
            if ((unsigned)f >= (unsigned)d.F) continue;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f, gt = 0.f;
            if (dL_dbary) { g0 = dL_dbary[3 * s]; g1 = dL_dbary[3 * s + 1]; g2 = dL_dbary[3 * s + 2]; }
            if (dL_dt) gt = dL_dt[s];
            if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f && gt == 0.0f) continue;
            const int64_t v[3] = {d.faces[3 * (int64_t)f], d.faces[3 * (int64_t)f + 1], d.faces[3 * (int64_t)f + 2]};
            double w[3], G[3];
            if (!rz_hit_grad(ro, rd, d.verts + 3 * v[0], d.verts + 3 * v[1], d.verts + 3 * v[2], g1 - g0, g2 - g0, gt, w, G)) continue;
            const int slot = tab.slot(f);
#pragma unroll
            for (int c = 0; c < RZ_NCOMP; c++) {
                const double gc = w[c / 3] * G[c % 3];
                if (gc == 0.0) continue;
                if (slot >= 0) tab.add(slot, c, gc);
                else atomicAdd(dL_dverts + 3 * v[c / 3] + c % 3, (float)gc);
            }
        }
    }
    __syncthreads();
    // flush: one global atomic per (vertex row, component) of every face the tile's pixels listed
    tab.flush_by_component(tid, [&](int f, int c, double sum) {
        const float g = (float)sum;
        if (g == 0.0f) return;                                           // a sum below fp32's range
        const int64_t v = d.faces[3 * (int64_t)f + c / 3];
        atomicAdd(dL_dverts + 3 * v + c % 3, g);
    });
}

// The overlap mode's backward.  Per listed slot: the fp32 intersection and clamp code of the forward, recomputed; then in fp64,
// with the code held fixed, (uc, vc) = clamp(u, v) and
//     code 0:  t = tuv.x                                    -> k_rasterize_bwd's slot, term for term;
//     else:    t = sum_k b_k d_k / rr,  b = (1 - uc - vc, uc, vc),  d_k = (p_k - ro) . rd,  rr = rd . rd, so
//              dL/duc = (g1 - g0) + g_t (d1 - d0) / rr,  dL/dvc = (g2 - g0) + g_t (d2 - d0) / rr,  and directly
//              dL/dp_k += g_t b_k rd / rr;
// (dL/du, dL/dv) = clamp_bary_uv_grad(code)^T (dL/duc, dL/dvc) goes through rz_hit_grad to the three vertices.
__global__ void __launch_bounds__(TILE_PIX)
k_rasterize_overlap_bwd(dm2_layers_desc d, dm2_window win, const int32_t* __restrict__ layers, const float* __restrict__ dL_dbary,
                        const float* __restrict__ dL_dt, float* __restrict__ dL_dverts) {
    __shared__ FaceTable<double, RZ_NCOMP> tab;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    tab.clear(tid);
    __syncthreads();

    const auto [px, py, inside, pix] = tile_pixel(tid, d.W, d.H);
    const WinOrigin org = window_origin(win.patch_min);
    if (inside) {
        f3 ro, rd;
        pixel_ray(d, b, pix, px + org.x, py + org.y, win.full_W, win.full_H, ro, rd);
        for (int l = 0; l < d.L; l++) {
            const int64_t s = pix * d.L + l;
            const int f = layers[s];
            if ((unsigned)f >= (unsigned)d.F) continue;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f, gt = 0.f;
            if (dL_dbary) { g0 = dL_dbary[3 * s]; g1 = dL_dbary[3 * s + 1]; g2 = dL_dbary[3 * s + 2]; }
            if (dL_dt) gt = dL_dt[s];
            if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f && gt == 0.0f) continue;
            const int64_t v[3] = {d.faces[3 * (int64_t)f], d.faces[3 * (int64_t)f + 1], d.faces[3 * (int64_t)f + 2]};
            const float* pa = d.verts + 3 * v[0];
            const float* pb = d.verts + 3 * v[1];
            const float* pc = d.verts + 3 * v[2];
            f3 tuv;
            if (!ray_tri_intersection(ro, rd, {pa[0], pa[1], pa[2]}, {pb[0], pb[1], pb[2]}, {pc[0], pc[1], pc[2]}, tuv)) continue;
            float uc32, vc32;
            int code;
            clamp_bary_uv(tuv.y, tuv.z, uc32, vc32, code);            // the forward's code, in the forward's fp32
            double guc = (double)g1 - (double)g0, gvc = (double)g2 - (double)g0, gtt = (double)gt, direct = 0.0;
            const double r3[3] = {rd.x, rd.y, rd.z};
            if (code != 0) {
                const double o3[3] = {ro.x, ro.y, ro.z};
                double d0 = 0.0, d1 = 0.0, d2 = 0.0, rr = 0.0;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    d0 += ((double)pa[i] - o3[i]) * r3[i]; d1 += ((double)pb[i] - o3[i]) * r3[i]; d2 += ((double)pc[i] - o3[i]) * r3[i];
                    rr += r3[i] * r3[i];
                }
                direct = (double)gt / rr;
                guc += direct * (d1 - d0);
                gvc += direct * (d2 - d0);
                gtt = 0.0;
            }
            float duc_du, duc_dv, dvc_du, dvc_dv;
            clamp_bary_uv_grad(code, duc_du, duc_dv, dvc_du, dvc_dv);
            const double gu = guc * (double)duc_du + gvc * (double)dvc_du, gv = guc * (double)duc_dv + gvc * (double)dvc_dv;
            double w[3], G[3];
            if (!rz_hit_grad<double>(ro, rd, pa, pb, pc, gu, gv, gtt, w, G)) continue;
            // the clamped barycentrics in fp64, the code held fixed (clamp_bary_uv's results per region)
            const double u = w[1], vv = w[2];
            const double uc = code == 1 || code == 3 || code == 4 ? 0.0 : (code == 2 ? 1.0 : (code == 6 ? (1.0 + u - vv) * 0.5 : u));
            const double vc = code == 1 || code == 2 || code == 5 ? 0.0 : (code == 3 ? 1.0 : (code == 6 ? (1.0 - u + vv) * 0.5 : vv));
            const double bc[3] = {1.0 - uc - vc, uc, vc};
            const int slot = tab.slot(f);
#pragma unroll
            for (int c = 0; c < RZ_NCOMP; c++) {
                const double gc = w[c / 3] * G[c % 3] + (direct * bc[c / 3]) * r3[c % 3];
                if (gc == 0.0) continue;
                if (slot >= 0) tab.add(slot, c, gc);
                else atomicAdd(dL_dverts + 3 * v[c / 3] + c % 3, (float)gc);
            }
        }
    }
    __syncthreads();
    tab.flush_by_component(tid, [&](int f, int c, double sum) {
        const float g = (float)sum;
        if (g == 0.0f) return;                                           // a sum below fp32's range
        const int64_t v = d.faces[3 * (int64_t)f + c / 3];
        atomicAdd(dL_dverts + 3 * v + c % 3, g);
    });
}

void launch_rasterize(const dm2_layers_desc& d, const dm2_window& win, const FaceState& fs, const uint2* ranges, const uint32_t* face_list,
                      int32_t* render_layers, int32_t* render_layers_cnt, float* bary, float* t, hipStream_t st) {
    const dim3 grid = tile_grid(d.W, d.H, d.B);
#define DM2_RZ_LAUNCH(KR) \
    hipLaunchKernelGGL(k_rasterize<KR>, grid, dim3(TILE_PIX), 0, st, d, win, fs.min_depths, fs.max_depths, ranges, face_list, \
                       render_layers, render_layers_cnt, bary, t)
    if (d.L <= 1) DM2_RZ_LAUNCH(1);
    else if (d.L <= 2) DM2_RZ_LAUNCH(2);
    else if (d.L <= 4) DM2_RZ_LAUNCH(4);
    else if (d.L <= 8) DM2_RZ_LAUNCH(8);
    else DM2_RZ_LAUNCH(16);
#undef DM2_RZ_LAUNCH
}

void launch_rasterize_backward(const dm2_layers_desc& d, const dm2_window& win, const int32_t* render_layers, const float* dL_dbary, const float* dL_dt,
                               float* dL_dverts, hipStream_t st) {
    const dim3 grid = tile_grid(d.W, d.H, d.B);
    hipLaunchKernelGGL(k_rasterize_bwd, grid, dim3(TILE_PIX), 0, st, d, win, render_layers, dL_dbary, dL_dt, dL_dverts);
}

void launch_rasterize_overlap(const dm2_layers_desc& d, const dm2_window& win, const uint2* ranges, const uint32_t* face_list,
                              int32_t* render_layers, int32_t* render_layers_cnt, float* bary, float* t, uint8_t* inside, hipStream_t st) {
    const dim3 grid = tile_grid(d.W, d.H, d.B);
#define DM2_RZO_LAUNCH(KR) \
    hipLaunchKernelGGL(k_rasterize_overlap<KR>, grid, dim3(TILE_PIX), 0, st, d, win, ranges, face_list, render_layers, \
                       render_layers_cnt, bary, t, inside)
    if (d.L <= 1) DM2_RZO_LAUNCH(1);
    else if (d.L <= 2) DM2_RZO_LAUNCH(2);
    else if (d.L <= 4) DM2_RZO_LAUNCH(4);
    else if (d.L <= 8) DM2_RZO_LAUNCH(8);
    else DM2_RZO_LAUNCH(16);
#undef DM2_RZO_LAUNCH
}

void launch_rasterize_overlap_backward(const dm2_layers_desc& d, const dm2_window& win, const int32_t* render_layers, const float* dL_dbary,
                                       const float* dL_dt, float* dL_dverts, hipStream_t st) {
    const dim3 grid = tile_grid(d.W, d.H, d.B);
    hipLaunchKernelGGL(k_rasterize_overlap_bwd, grid, dim3(TILE_PIX), 0, st, d, win, render_layers, dL_dbary, dL_dt, dL_dverts);
}

}  // namespace dm2
