// dm2_tex_core.h -- what the three texture ops share (dm2_texture.hip, dm2_texture_mip.hip, dm2_texture_cube.hip): the
// constants, the addressing and the four taps of one level, the bilinear blend and its coordinate gradient, the forward's
// sweep, the tile scatter of the texel gradients, and the launchers' small change.  (The empty-slot test of a uv pair is three
// lines in tx_tap and in tm_tap: as a function here it changed the forwards' instruction streams.)
// Each op keeps how a slot becomes taps (its *Tap struct and *_tap function) and its kernels; what differs between the ops
// inside a shared piece is a template parameter or a callable, never a run-time test of which op is calling.
// -ffp-contract=off: every formula here is its written operation order, and the forwards are pinned to it bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"

namespace dm2 {

constexpr int TEX_BLOCK = 256;            // slots per block of the flat kernels
constexpr int TEX_CH = 4;                 // the longest channel chunk of the tex backwards
constexpr int TEX_NEAREST = 0, TEX_LINEAR = 1;    // DM2_TEX_FILTER_*
constexpr int TEX_WRAP = 0, TEX_CLAMP = 1;        // DM2_TEX_BOUNDARY_*
constexpr float TEX_RANGE = 16777216.0f;  // 2^24: beyond it the integer conversion and the fraction mean nothing
// the scatter's FaceTable: CH fp32 accumulators per slot; flush: bank = (c * (64 / CH) + slot) % 64
template <int CH> constexpr int TEX_STRIDE = LC_SLOTS + (64 + CH - 1) / CH;
template <int CH> using TexTable = FaceTable<float, CH, TEX_STRIDE<CH>>;

template <int BOUNDARY>
__device__ __forceinline__ int tex_addr(int i, int n) {
    if (BOUNDARY == TEX_CLAMP) return min(max(i, 0), n - 1);
    const int r = i % n;                  // ((i % n) + n) % n without the sum that overflows for n > 2^30
    return r < 0 ? r + n : r;
}

// the taps t00, t10, t01, t11 of a Wk x Hk level at (x, y) as indices base + j * Wk + i, and the fractions
template <int BOUNDARY>
__device__ __forceinline__ void tex_linear_taps(int Wk, int Hk, int base, float x, float y, int (&idx)[4], float& fx, float& fy) {
    const float x0 = floorf(x), y0 = floorf(y);
    fx = x - x0; fy = y - y0;
    const int i0 = (int)x0, j0 = (int)y0;
    const int a0 = tex_addr<BOUNDARY>(i0, Wk), a1 = tex_addr<BOUNDARY>(i0 + 1, Wk);
    const int r0 = base + tex_addr<BOUNDARY>(j0, Hk) * Wk, r1 = base + tex_addr<BOUNDARY>(j0 + 1, Hk) * Wk;
    idx[0] = r0 + a0; idx[1] = r0 + a1; idx[2] = r1 + a0; idx[3] = r1 + a1;
}

__device__ __forceinline__ float tex_bilinear(float t00, float t10, float t01, float t11, float fx, float fy) {
    const float a = t00 + fx * (t10 - t00), b = t01 + fx * (t11 - t01);
    return a + fy * (b - a);
}

// one channel's terms of sum_c g d out / d fx and sum_c g d out / d fy
__device__ __forceinline__ void tex_uv_term(float t00, float t10, float t01, float t11, float g, float fx, float fy, float& su, float& sv) {
    const float d0 = t10 - t00, d1 = t11 - t01;
    const float a = t00 + fx * d0, b = t01 + fx * d1;
    su += g * (d0 + fy * (d1 - d0));
    sv += g * (b - a);
}

// VEC4 everywhere below: C is a multiple of 4 and the tensors are 16-byte aligned, so a lane takes four channels at a time;
// every channel goes through the same operations either way (the same bits).  The scalar path uses x alone.
// TexQuad travels by value: a kernel whose result is written through a reference by something it calls compiles the blend of
// the four channels into fewer packed instructions (k_texture<linear, .., true>: 7 instructions more).
struct TexQuad { float x, y, z, w; };

template <bool VEC4>
__device__ __forceinline__ TexQuad tex_load_row(const float* p) {
    if (VEC4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        return {t.x, t.y, t.z, t.w};
    }
    return {*p, 0.0f, 0.0f, 0.0f};
}

// the bilinear blend of the four taps' channels
template <bool VEC4>
__device__ __forceinline__ TexQuad tex_blend_rows(TexQuad t00, TexQuad t10, TexQuad t01, TexQuad t11, float fx, float fy) {
    if (VEC4)
        return {tex_bilinear(t00.x, t10.x, t01.x, t11.x, fx, fy), tex_bilinear(t00.y, t10.y, t01.y, t11.y, fx, fy),
                tex_bilinear(t00.z, t10.z, t01.z, t11.z, fx, fy), tex_bilinear(t00.w, t10.w, t01.w, t11.w, fx, fy)};
    return {tex_bilinear(t00.x, t10.x, t01.x, t11.x, fx, fy), 0.0f, 0.0f, 0.0f};
}

// ... loaded from the rows at p00 .. p11
template <bool VEC4>
__device__ __forceinline__ TexQuad tex_sample_rows(const float* p00, const float* p10, const float* p01, const float* p11, float fx, float fy) {
    return tex_blend_rows<VEC4>(tex_load_row<VEC4>(p00), tex_load_row<VEC4>(p10), tex_load_row<VEC4>(p01), tex_load_row<VEC4>(p11), fx, fy);
}

// The forward's sweep over a block's nslots * C outputs (the block's first slot is s0), after each lane staged one slot in
// LDS (idx0[slot] < 0: empty, zeros out): consecutive lanes on consecutive floats (four floats per lane on the vector path), so
// the stores of a wave are contiguous and the lanes of one slot read consecutive channels of the same texels.
// sample(slot, i00, c): the V channels from c * V of a live slot.
template <bool VEC4, typename Sample>
__device__ __forceinline__ void tex_sweep(int tid, int nslots, int C, const int* idx0, float* out, int64_t s0, Sample&& sample) {
    constexpr int V = VEC4 ? 4 : 1;
    const int CV = C / V, total = nslots * CV;                                // lane -> (slot, group of V channels), group fastest
    const int dq = TEX_BLOCK / CV, dr = TEX_BLOCK - dq * CV;                  // the step of (slot, group) per sweep
    int slot = tid / CV, c = tid - slot * CV;
    float* o = out + s0 * C;
    for (int e = tid; e < total; e += TEX_BLOCK) {
        const int i00 = idx0[slot];
        TexQuad r = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i00 >= 0) r = sample(slot, i00, c);
        if (VEC4) reinterpret_cast<float4*>(o)[e] = make_float4(r.x, r.y, r.z, r.w);
        else o[e] = r.x;
        slot += dq; c += dr;
        if (c >= CV) { c -= CV; slot++; }
    }
}

// The tex backwards' scatter, one layer of one tile: lane tid's slot s adds w[k] * g[s, c] to channel c of texel key[k] for
// its first nt of NT (key, weight) pairs, but for pair ``skip`` (-1: none), when live.  One block per 16 x 16 pixel tile and view,
// one lane per pixel, one layer at a time (slot l of neighbouring pixels is usually one surface, so its texels are neighbours;
// the L slots of a pixel are unrelated texels), the channels of the layer in chunks of CH.
// A contribution goes into the texel's slot of the block's table, keyed by the op's texel index, and the table is flushed by
// slot: consecutive lanes on consecutive channels of one texel, one global atomic per (texel, channel) it holds.  Under
// minification a tile touches up to 1024 distinct texels per layer, and straight to global memory is then the usual route.
// The table is cleared for every layer (a table kept across the layers of a tile fills up with the first layers' texels and
// measured 1.1-2x slower); within a layer the keys stay from chunk to chunk, so a texel keeps its slot.
// (k_texture_mip_bwd_tex and k_texture_cube_bwd_tex call this; k_texture_bwd_tex has the same body written out: see there.)
// row(key): texel key's row of C floats in its gradient tensor.  MAY_BE_ABSENT: row() may return null for a tensor that is
// not wanted, and that pair is skipped (a key the table holds has a row).
template <int CH, int NT, bool MAY_BE_ABSENT, typename Row>
__device__ __forceinline__ void tex_scatter_layer(TexTable<CH>& tab, int tid, bool live, const int* key, const float* w, int nt, int skip,
                                                  const float* __restrict__ g, int64_t s, int C, Row&& row) {
    tab.clear_keys(tid);
    for (int c0 = 0; c0 < C; c0 += CH) {
        const int nc = min(CH, C - c0);
        tab.clear_acc(tid);
        __syncthreads();
        if (live) {
            float gv[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) gv[c] = c < nc ? g[s * C + c0 + c] : 0.0f;
#pragma unroll
            for (int k = 0; k < NT; k++) {
                if (k >= nt || k == skip) continue;
                float* dst = row(key[k]);
                if (MAY_BE_ABSENT && !dst) continue;
                const int slot = tab.slot(key[k]);
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    if (c >= nc) continue;
                    const float v = w[k] * gv[c];
                    if (slot >= 0) tab.add(slot, c, v);
                    else atomicAdd(dst + c0 + c, v);
                }
            }
        }
        __syncthreads();
        tab.flush_by_slot(tid, [&](int k, int c, float v) {
            if (c < nc) atomicAdd(row(k) + c0 + c, v);
        });
        __syncthreads();
    }
}

// tex_scatter_layer for a caller whose list has holes: pair k takes part when bit k of ``mask`` is set (the cube's mip chain: a
// corner's missing tap, one per level at the most, so a single ``skip`` does not say it).  The same body otherwise; written
// out a second time because tex_scatter_layer's callers are pinned to their instruction streams.
// ``first``: the pairs (bits of mask) whose keys claim their table slots before any other key does.  A tile of unrelated
// directions holds up to 8 * 256 keys, four times the table; the keys of the coarse levels are the few that every tile of the
// frame shares, and one of them that finds the table full would go to global memory once per lane, all on the same addresses.
template <int CH, int NT, bool MAY_BE_ABSENT, typename Row>
__device__ __forceinline__ void tex_scatter_layer_masked(TexTable<CH>& tab, int tid, bool live, const int* key, const float* w, unsigned mask,
                                                         unsigned first, const float* __restrict__ g, int64_t s, int C, Row&& row) {
    tab.clear_keys(tid);
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < NT; k++) {
            if (!((mask & first) >> k & 1u)) continue;
            if (MAY_BE_ABSENT && !row(key[k])) continue;
            tab.slot(key[k]);
        }
    }
    for (int c0 = 0; c0 < C; c0 += CH) {
        const int nc = min(CH, C - c0);
        tab.clear_acc(tid);
        __syncthreads();
        if (live) {
            float gv[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) gv[c] = c < nc ? g[s * C + c0 + c] : 0.0f;
#pragma unroll
            for (int k = 0; k < NT; k++) {
                if (!((mask >> k) & 1u)) continue;
                float* dst = row(key[k]);
                if (MAY_BE_ABSENT && !dst) continue;
                const int slot = tab.slot(key[k]);
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    if (c >= nc) continue;
                    const float v = w[k] * gv[c];
                    if (slot >= 0) tab.add(slot, c, v);
                    else atomicAdd(dst + c0 + c, v);
                }
            }
        }
        __syncthreads();
        tab.flush_by_slot(tid, [&](int k, int c, float v) {
            if (c < nc) atomicAdd(row(k) + c0 + c, v);
        });
        __syncthreads();
    }
}

// ---- host side ----

// the fields every op's sizes struct has
template <typename Z>
static void tex_common_sizes(Z& z, int B, int H, int W, int L, int C, int view_textures) {
    z.per_view = (int64_t)H * W * L;
    z.S = (int64_t)B * z.per_view;
    z.B = B; z.H = H; z.W = W; z.L = L; z.C = C; z.view_textures = view_textures;
}

template <typename... P>
static bool tex_aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }

// one lane per element, TEX_BLOCK lanes per block
static inline dim3 tex_flat_grid(int64_t n, unsigned views = 1) { return dim3((unsigned)((n + TEX_BLOCK - 1) / TEX_BLOCK), views); }

// X(F, Bd) with the call's runtime (filter, boundary) as compile-time constants, for the op that has both; the ops with one
// mode write their if / else out
#define DM2_TEX_MODES(filter, boundary, X)                                  \
    do {                                                                    \
        if ((filter) == TEX_LINEAR) {                                       \
            if ((boundary) == TEX_WRAP) { X(TEX_LINEAR, TEX_WRAP); } else { X(TEX_LINEAR, TEX_CLAMP); }   \
        } else {                                                            \
            if ((boundary) == TEX_WRAP) { X(TEX_NEAREST, TEX_WRAP); } else { X(TEX_NEAREST, TEX_CLAMP); } \
        }                                                                   \
    } while (0)

// X(..., CH) with the chunk length of a C-channel tex backward as a compile-time constant
#define DM2_TEX_CHUNK(C, X, ...)                    \
    do {                                            \
        if ((C) == 1) { X(__VA_ARGS__, 1); }        \
        else if ((C) == 2) { X(__VA_ARGS__, 2); }   \
        else if ((C) == 3) { X(__VA_ARGS__, 3); }   \
        else { X(__VA_ARGS__, TEX_CH); }            \
    } while (0)

}  // namespace dm2
