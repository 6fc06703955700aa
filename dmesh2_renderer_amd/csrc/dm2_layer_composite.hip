// dm2_layer_composite.hip -- the differentiable consumer of LayeredRenderer's layers:
//   k_layer_composite      front-to-back alpha compositing of caller-supplied per-pixel face lists
//   k_layer_composite_bwd  its gradients w.r.t. verts_color, faces_opacity, faces_intense and verts_ndc (z)
//
// Contract (include/dm2_hip.h, dm2_layers_composite): per pixel T = 1, C = D = 0; for l = 0..L-1, f = render_layers[.., l]:
// skip f outside [0, F); intersect the pixel's ray with verts[faces[f]] (ray_tri_intersection), skip an edge case; skip
// unless clamp_bary_uv's code is 0 (Renderer's coverage at aa_temperature 0); then colour, depth and alpha in the
// operation order of the point-sampled forward (dm2_forward_point.hip, forward.cu:380-395) and the same blend; stop once
// T < T_EPS.  color = C + T * background, depth_raw = D + T.  -ffp-contract=off (Makefile): the forward is bit-exact.
//
// Layout of both kernels: one lane per pixel, 16 x 16 tiles, the view on blockIdx.z (as k_first_intersect).  A layer costs
// direct gathers (face ids, 9 world coordinates, 9 colours, 3 z, opacity, intensity): no per-(view, face) record is
// packed -- see DESIGN.md on why that was not built.
//
// Backward.  No division by (1 - alpha): opacities here are existence probabilities and reach 1.0.  With the colour behind
// layer l, R_l = alpha_l iC_l + (1 - alpha_l) R_{l+1} (R after the last contributing layer = background; depth: 1),
//     dL/dalpha_l = T_l (g_c . (iC_l - R_{l+1}) + g_d (iD_l - RD_{l+1})),
// with T_l from a front-to-back pass.  The layers [0, n_contrib) are processed in chunks of LC_REG from the back: per chunk
// a front pass (T at the chunk's start from the layers in front of it, then the chunk's hits kept in registers) and a back
// pass that carries R.  L <= LC_REG is one chunk; a larger L re-intersects the layers in front of each chunk (correct, not fast).
// ALPHA (the template parameter; dm2_layers_composite_backward with dL_dout_alpha): the alpha image 1 - T_final is a fourth channel of
// colour 1 over background 0, RA_l = alpha_l + (1 - alpha_l) RA_{l+1} (RA = 0 behind the last layer), and adds
// T_l g_A (1 - RA_{l+1}) to dL/dalpha_l -- still no division.
//
// Gradient scatter: a (pixel, layer) hit adds its 14 components (9 colour, 3 z, opacity, intensity) into the block's
// FaceTable (dm2_face_table.h) under its face id; the flush is one global atomic per (face or vertex row, component).
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_stage.h"
#include "dm2_state.h"

namespace dm2 {

constexpr int LC_REG = 8;          // layers of a chunk held in registers by the backward
constexpr int LC_NCOMP = 14;       // d colour (3 vertices x 3 channels), d z (3), d opacity, d intensity
constexpr int LC_DZ = 9, LC_OP = 12, LC_IN = 13;

// one layer of one pixel: the contract's steps 1-4.  false: the layer is skipped.
struct LcHit { float u, v, bc0, bc1, bc2, intense, iD, alpha; };

__device__ __forceinline__ bool lc_layer(const dm2_layer_composite_desc& d, int b, int f, f3 ro, f3 rd, LcHit& h) {
    if ((unsigned)f >= (unsigned)d.F) return false;
    const int64_t v0 = d.faces[3 * (int64_t)f], v1 = d.faces[3 * (int64_t)f + 1], v2 = d.faces[3 * (int64_t)f + 2];
    const f3 p0 = {d.verts[3 * v0], d.verts[3 * v0 + 1], d.verts[3 * v0 + 2]};
    const f3 p1 = {d.verts[3 * v1], d.verts[3 * v1 + 1], d.verts[3 * v1 + 2]};
    const f3 p2 = {d.verts[3 * v2], d.verts[3 * v2 + 1], d.verts[3 * v2 + 2]};
    f3 tuv = {0, 0, 0};
    if (!ray_tri_intersection(ro, rd, p0, p1, p2, tuv)) return false;
    float iuc, ivc;
    int code;
    clamp_bary_uv(tuv.y, tuv.z, iuc, ivc, code);
    if (code != 0) return false;
    const float i0 = 1 - iuc - ivc, i1 = iuc, i2 = ivc;
    const float* c = d.verts_color;
    h.u = iuc; h.v = ivc;
    h.bc0 = i0 * c[3 * v0] + i1 * c[3 * v1] + i2 * c[3 * v2];
    h.bc1 = i0 * c[3 * v0 + 1] + i1 * c[3 * v1 + 1] + i2 * c[3 * v2 + 1];
    h.bc2 = i0 * c[3 * v0 + 2] + i1 * c[3 * v1 + 2] + i2 * c[3 * v2 + 2];
    h.intense = d.faces_intense[(int64_t)b * d.F + f];
    const float* z = d.verts_ndc + (int64_t)b * d.P * 3 + 2;
    h.iD = i0 * z[3 * v0] + i1 * z[3 * v1] + i2 * z[3 * v2];
    h.alpha = d.faces_opacity[f];
    return true;
}

// one pixel of k_layer_composite (WEIGHTS: its blends' alpha * T into the block's table)
template <int VEC, bool WEIGHTS>
__device__ __forceinline__ void lc_composite_pixel(const dm2_layer_composite_desc& d, const dm2_window& win, int b, uint32_t px, uint32_t py,
                                                   float* __restrict__ out_color, float* __restrict__ out_depth,
                                                   float* __restrict__ out_final_T, int32_t* __restrict__ out_n_contrib,
                                                   float* __restrict__ face_weights, FaceTable<float, 1>* tab) {
    const int64_t pix = ((int64_t)b * d.H + py) * d.W + px;
    // (a window: only the analytic ray needs the origin; the ray tensors are the window's own)
    const WinOrigin org = window_origin(win.patch_min);
    f3 ro, rd;
    pixel_ray(d, b, pix, px + org.x, py + org.y, win.full_W, win.full_H, ro, rd);
    const int32_t* ids = d.render_layers + pix * d.L;
    float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f;
    int n_contrib = 0;
    bool done = false;
    auto blend = [&](int l, int f) {
        LcHit h;
        if (!lc_layer(d, b, f, ro, rd, h)) return;
        const float c0 = h.bc0 * h.intense, c1 = h.bc1 * h.intense, c2 = h.bc2 * h.intense;
        const float alpha = h.alpha;
        const float test_T = T * (1 - alpha);
        if constexpr (WEIGHTS) {
            tab->add_or(tab->slot(f), 0, alpha * T, face_weights + (int64_t)b * d.F + f);
        }
        C0 += c0 * alpha * T; C1 += c1 * alpha * T; C2 += c2 * alpha * T;
        D += h.iD * alpha * T;
        T = test_T;
        n_contrib = l + 1;
        if (T < T_EPS) done = true;
    };
    for (int l = 0; l < d.L && !done; l += VEC) {
        if (VEC == 4) {
            const int4 q = *reinterpret_cast<const int4*>(ids + l);
            blend(l, q.x);
            if (!done) blend(l + 1, q.y);
            if (!done) blend(l + 2, q.z);
            if (!done) blend(l + 3, q.w);
        } else if (VEC == 2) {
            const int2 q = *reinterpret_cast<const int2*>(ids + l);
            blend(l, q.x);
            if (!done) blend(l + 1, q.y);
        } else {
            blend(l, ids[l]);
        }
    }
    out_color[3 * pix] = C0 + T * d.background[0];
    out_color[3 * pix + 1] = C1 + T * d.background[1];
    out_color[3 * pix + 2] = C2 + T * d.background[2];
    out_depth[pix] = D + T * 1.0f;
    if (out_final_T) out_final_T[pix] = T;
    if (out_n_contrib) out_n_contrib[pix] = n_contrib;
}

// WEIGHTS (dm2_layers_composite with out_face_weights): every blend adds its alpha * T into a FaceTable of one accumulator per face, flushed
// with one global atomic per (block, face).  Without WEIGHTS no table is declared.
template <int VEC, bool WEIGHTS>
__global__ void __launch_bounds__(TILE_PIX)
k_layer_composite(dm2_layer_composite_desc d, dm2_window win, float* __restrict__ out_color, float* __restrict__ out_depth,
                  float* __restrict__ out_final_T, int32_t* __restrict__ out_n_contrib, float* __restrict__ face_weights) {
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const TilePixel t = tile_pixel(tid, d.W, d.H);
    if constexpr (WEIGHTS) {
        __shared__ FaceTable<float, 1> tab;
        tab.clear(tid);
        __syncthreads();
        if (t.inside) lc_composite_pixel<VEC, true>(d, win, b, t.px, t.py, out_color, out_depth, out_final_T, out_n_contrib, face_weights, &tab);
        __syncthreads();
        tab.flush_by_slot(tid, [&](int f, int, float w) { atomicAdd(face_weights + (int64_t)b * d.F + f, w); });
    } else {
        if (!t.inside) return;
        lc_composite_pixel<VEC, false>(d, win, b, t.px, t.py, out_color, out_depth, out_final_T, out_n_contrib, nullptr, nullptr);
    }
}

struct LcGrads {
    float* dcolor;      // (P,3)
    float* dopacity;    // (F)
    float* dndc;        // (B,P,3), z only
    float* dintense;    // (B,F)
};

__device__ __forceinline__ void lc_global_add(const dm2_layer_composite_desc& d, int b, int f, const float* g, const LcGrads& o) {
    const int v[3] = {d.faces[3 * (int64_t)f], d.faces[3 * (int64_t)f + 1], d.faces[3 * (int64_t)f + 2]};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            if (g[3 * i + ch] != 0.0f) atomicAdd(o.dcolor + 3 * (int64_t)v[i] + ch, g[3 * i + ch]);
        if (g[LC_DZ + i] != 0.0f) atomicAdd(o.dndc + ((int64_t)b * d.P + v[i]) * 3 + 2, g[LC_DZ + i]);
    }
    if (g[LC_OP] != 0.0f) atomicAdd(o.dopacity + f, g[LC_OP]);
    if (g[LC_IN] != 0.0f) atomicAdd(o.dintense + (int64_t)b * d.F + f, g[LC_IN]);
}

template <bool ALPHA>
__global__ void __launch_bounds__(TILE_PIX)
k_layer_composite_bwd(dm2_layer_composite_desc d, dm2_window win, const float* __restrict__ dL_dcolor, const float* __restrict__ dL_ddepth,
                      const int32_t* __restrict__ n_contrib, LcGrads o, const float* __restrict__ dL_dalpha) {
    __shared__ FaceTable<float, LC_NCOMP> tab;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    tab.clear(tid);
    __syncthreads();

    const auto [px, py, inside, pix] = tile_pixel(tid, d.W, d.H);
    const int n = inside ? min(n_contrib[pix], d.L) : 0;
    if (n > 0) {
        const WinOrigin org = window_origin(win.patch_min);
        f3 ro, rd;
        pixel_ray(d, b, pix, px + org.x, py + org.y, win.full_W, win.full_H, ro, rd);
        const int32_t* ids = d.render_layers + pix * d.L;
        const float g0 = dL_dcolor[3 * pix], g1 = dL_dcolor[3 * pix + 1], g2 = dL_dcolor[3 * pix + 2], gd = dL_ddepth[pix];
        float R0 = d.background[0], R1 = d.background[1], R2 = d.background[2], RD = 1.0f;
        float gA = 0.f, RA = 0.f;                                       // (ALPHA only)
        if constexpr (ALPHA) gA = dL_dalpha[pix];
        for (int e = n; e > 0;) {
            const int s = e > LC_REG ? e - LC_REG : 0;
            float T = 1.0f;
            for (int l = 0; l < s; l++) {                                // (L > LC_REG only) T in front of the chunk
                LcHit h;
                if (lc_layer(d, b, ids[l], ro, rd, h)) T = T * (1 - h.alpha);
            }
            LcHit hs[LC_REG];
            float Ts[LC_REG];
            bool hit[LC_REG];
            int fs[LC_REG];
#pragma unroll
            for (int j = 0; j < LC_REG; j++) {
                const int l = s + j;
                fs[j] = l < e ? ids[l] : -1;
                hit[j] = l < e && lc_layer(d, b, fs[j], ro, rd, hs[j]);
                Ts[j] = T;
                if (hit[j]) T = T * (1 - hs[j].alpha);
            }
#pragma unroll
            for (int j = LC_REG - 1; j >= 0; j--) {
                if (!hit[j]) continue;
                const LcHit& h = hs[j];
                const float c0 = h.bc0 * h.intense, c1 = h.bc1 * h.intense, c2 = h.bc2 * h.intense;
                const float aT = h.alpha * Ts[j];
                const float w[3] = {1 - h.u - h.v, h.u, h.v};
                float g[LC_NCOMP];
                const float gc0 = g0 * aT * h.intense, gc1 = g1 * aT * h.intense, gc2 = g2 * aT * h.intense, gz = gd * aT;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    g[3 * i] = gc0 * w[i]; g[3 * i + 1] = gc1 * w[i]; g[3 * i + 2] = gc2 * w[i];
                    g[LC_DZ + i] = gz * w[i];
                }
                g[LC_OP] = Ts[j] * ((g0 * (c0 - R0) + g1 * (c1 - R1) + g2 * (c2 - R2)) + gd * (h.iD - RD));
                if constexpr (ALPHA) {
                    g[LC_OP] += Ts[j] * gA * (1 - RA);
                    RA = h.alpha + (1 - h.alpha) * RA;
                }
                g[LC_IN] = (g0 * h.bc0 + g1 * h.bc1 + g2 * h.bc2) * aT;
                const float om = 1 - h.alpha;
                R0 = h.alpha * c0 + om * R0; R1 = h.alpha * c1 + om * R1; R2 = h.alpha * c2 + om * R2;
                RD = h.alpha * h.iD + om * RD;
                const int slot = tab.slot(fs[j]);
                if (slot >= 0) {
#pragma unroll
                    for (int c = 0; c < LC_NCOMP; c++)
                        if (g[c] != 0.0f) tab.add(slot, c, g[c]);
                } else {
                    lc_global_add(d, b, fs[j], g, o);
                }
            }
            e = s;
        }
    }
    __syncthreads();
    // flush: one global atomic per (face or vertex row, component) of every face the tile's pixels hit
    tab.flush_by_component(tid, [&](int f, int c, float g) {
        if (c == LC_OP) { atomicAdd(o.dopacity + f, g); return; }
        if (c == LC_IN) { atomicAdd(o.dintense + (int64_t)b * d.F + f, g); return; }
        const int vi = c < LC_DZ ? c / 3 : c - LC_DZ;
        const int64_t v = d.faces[3 * (int64_t)f + vi];
        if (c < LC_DZ) atomicAdd(o.dcolor + 3 * v + (c - 3 * vi), g);
        else atomicAdd(o.dndc + ((int64_t)b * d.P + v) * 3 + 2, g);
    });
}

void launch_layer_composite(const dm2_layer_composite_desc& d, const dm2_window& win, float* out_color, float* out_depth, float* out_final_T,
                            int32_t* out_n_contrib, float* out_face_weights, hipStream_t st) {
    const dim3 grid = tile_grid(d.W, d.H, d.B);
    // layer ids as 16- or 8-byte vectors where L and the pointer allow it
    const uintptr_t a = (uintptr_t)d.render_layers;
    const int vec = (d.L % 4 == 0 && a % 16 == 0) ? 4 : (d.L % 2 == 0 && a % 8 == 0) ? 2 : 1;
#define DM2_LC_LAUNCH(V, W) \
    hipLaunchKernelGGL((k_layer_composite<V, W>), grid, dim3(TILE_PIX), 0, st, d, win, out_color, out_depth, out_final_T, out_n_contrib, out_face_weights)
    if (out_face_weights) {
        if (vec == 4) DM2_LC_LAUNCH(4, true); else if (vec == 2) DM2_LC_LAUNCH(2, true); else DM2_LC_LAUNCH(1, true);
    } else {
        if (vec == 4) DM2_LC_LAUNCH(4, false); else if (vec == 2) DM2_LC_LAUNCH(2, false); else DM2_LC_LAUNCH(1, false);
    }
#undef DM2_LC_LAUNCH
}

void launch_layer_composite_backward(const dm2_layer_composite_desc& d, const dm2_window& win, const float* dL_dcolor, const float* dL_ddepth,
                                     const int32_t* n_contrib, float* dL_dverts_color, float* dL_dfaces_opacity,
                                     float* dL_dverts_ndc, float* dL_dfaces_intense, const float* dL_dalpha, hipStream_t st) {
    const dim3 grid = tile_grid(d.W, d.H, d.B);
    const LcGrads o{dL_dverts_color, dL_dfaces_opacity, dL_dverts_ndc, dL_dfaces_intense};
    if (dL_dalpha)
        hipLaunchKernelGGL(k_layer_composite_bwd<true>, grid, dim3(TILE_PIX), 0, st, d, win, dL_dcolor, dL_ddepth, n_contrib, o, dL_dalpha);
    else
        hipLaunchKernelGGL(k_layer_composite_bwd<false>, grid, dim3(TILE_PIX), 0, st, d, win, dL_dcolor, dL_ddepth, n_contrib, o, dL_dalpha);
}

}  // namespace dm2
