// dm2_texture.hip -- Renderer.texture: a channel-last texture sampled at interpolate's UVs, per slot s = (b, y, x, l):
//   k_texture            out[s, c] = a + fy (b - a),  a = t00 + fx (t10 - t00),  b = t01 + fx (t11 - t01)   (nearest: one texel)
//   k_texture_bwd_uv     dL/du[s] = Wt sum_c g[s,c] (d0 + fy (d1 - d0)),  dL/dv[s] = Ht sum_c g[s,c] (b - a),  d0 = t10 - t00, d1 = t11 - t01
//   k_texture_bwd_tex    dL/dtex[t_pq, c] += w_pq g[s, c]
//
// Contract (include/dm2_hip.h, dm2_texture): x = u * Wt - 0.5, y = v * Ht - 0.5 in fp32 (texel centres at (i + 0.5) / Wt);
// x0 = floor(x), fx = x - x0; a slot is empty when its id is negative or |x| or |y| is not below 2^24 (NaN and infinite uv
// included): zeros out, nothing read from tex through it, no gradient.  -ffp-contract=off: the forward is a pure function of
// the written operation order.
//
// Forward: the slots are a flat list.  A block takes 256 consecutive slots; each lane computes one slot's texel indices and
// fractions once and stages them in LDS, then the block sweeps its 256 * C outputs with consecutive lanes on consecutive
// floats (four floats per lane on the vector path): the stores of a wave are contiguous and the lanes of one slot read
// consecutive channels of the same four texels.
//
// uv backward: one lane per slot, a sequential fp32 sum over the channels, two plain stores.
//
// tex backward: the scatter.  One block per 16 x 16 pixel tile and view, one lane per pixel, one layer at a time (slot l of
// neighbouring pixels is usually one surface, so its texels are neighbours; the L slots of a pixel are unrelated texels), the
// channels of a layer in chunks of CH.
// A (slot, corner, channel) contribution goes into the texel's slot of the block's FaceTable (dm2_face_table.h), keyed by the
// texel's linear index j * Wt + i (CH fp32 accumulators per slot, a stride that keeps the 64 lanes of the flush in 64 banks),
// flushed by slot: consecutive lanes on consecutive channels of one texel.  Under minification a tile touches up to 1024
// distinct texels per layer, and straight to global memory is then the usual route.  The table is cleared for every layer (a table
// kept across the layers of a tile fills up with the first layers' texels and measured 1.1-2x slower); within a
// layer the keys stay from chunk to chunk, so a texel keeps its slot.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"

namespace dm2 {

constexpr int TX_BLOCK = 256;             // slots per block of the flat kernels
constexpr int TX_CH = 4;                  // the longest channel chunk of the tex backward
constexpr int TX_NEAREST = 0, TX_LINEAR = 1;      // DM2_TEX_FILTER_*
constexpr int TX_WRAP = 0, TX_CLAMP = 1;          // DM2_TEX_BOUNDARY_*
constexpr float TX_RANGE = 16777216.0f;   // 2^24: beyond it the integer conversion and the fraction mean nothing

struct TexSizes {
    int64_t S;        // B * H * W * L slots
    int64_t per_view; // slots per view (H * W * L)
    int64_t texels;   // Ht * Wt (< 2^31)
    int B, H, W, L, Ht, Wt, C;
    int view_textures; // tex is (B, Ht, Wt, C): texel t of view b is texel b * Ht * Wt + t
};

// one slot's sample: texel indices j * Wt + i of the corners (t00, t10, t01, t11; nearest: idx[0] alone) and the fractions
struct TexTap {
    int idx[4];
    float fx, fy;
};

template <int BOUNDARY>
__device__ __forceinline__ int tx_addr(int i, int n) {
    if (BOUNDARY == TX_CLAMP) return min(max(i, 0), n - 1);
    const int r = i % n;                  // ((i % n) + n) % n without the sum that overflows for n > 2^30
    return r < 0 ? r + n : r;
}

// false = empty slot (nothing of ``tap`` is set)
template <int FILTER, int BOUNDARY>
__device__ __forceinline__ bool tx_tap(const TexSizes& z, int64_t s, const int32_t* __restrict__ layers,
                                       const float* __restrict__ uv, TexTap& tap) {
    if (layers && layers[s] < 0) return false;
    const float u = uv[2 * s], v = uv[2 * s + 1];
    const float x = u * (float)z.Wt - 0.5f, y = v * (float)z.Ht - 0.5f;
    if (!(fabsf(x) < TX_RANGE) || !(fabsf(y) < TX_RANGE)) return false;          // NaN and infinities included
    if (FILTER == TX_NEAREST) {
        const int i = tx_addr<BOUNDARY>((int)floorf(x + 0.5f), z.Wt), j = tx_addr<BOUNDARY>((int)floorf(y + 0.5f), z.Ht);
        tap.idx[0] = j * z.Wt + i;
        tap.idx[1] = tap.idx[2] = tap.idx[3] = tap.idx[0];
        tap.fx = tap.fy = 0.0f;
        return true;
    }
    const float x0 = floorf(x), y0 = floorf(y);
    tap.fx = x - x0; tap.fy = y - y0;
    const int i0 = (int)x0, j0 = (int)y0;
    const int a0 = tx_addr<BOUNDARY>(i0, z.Wt), a1 = tx_addr<BOUNDARY>(i0 + 1, z.Wt);
    const int r0 = tx_addr<BOUNDARY>(j0, z.Ht) * z.Wt, r1 = tx_addr<BOUNDARY>(j0 + 1, z.Ht) * z.Wt;
    tap.idx[0] = r0 + a0; tap.idx[1] = r0 + a1; tap.idx[2] = r1 + a0; tap.idx[3] = r1 + a1;
    return true;
}

__device__ __forceinline__ float tx_bilinear(float t00, float t10, float t01, float t11, float fx, float fy) {
    const float a = t00 + fx * (t10 - t00), b = t01 + fx * (t11 - t01);
    return a + fy * (b - a);
}

// VEC4: C is a multiple of 4 and tex / out are 16-byte aligned, so a lane takes four channels at a time; every channel goes
// through the same operations either way (the same bits).
template <int FILTER, int BOUNDARY, bool VEC4>
__global__ void __launch_bounds__(TX_BLOCK)
k_texture(TexSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ tex,
          float* __restrict__ out) {
    constexpr int NIDX = FILTER == TX_LINEAR ? 4 : 1;
    __shared__ int s_idx[NIDX][TX_BLOCK];                                     // idx[0] < 0: empty slot
    __shared__ float s_fx[TX_BLOCK], s_fy[TX_BLOCK];
    __shared__ int s_view[TX_BLOCK];
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * TX_BLOCK;
    const int nslots = (int)min((int64_t)TX_BLOCK, z.S - s0);
    if (tid < nslots) {
        const int64_t s = s0 + tid;
        TexTap tap;
        const bool ok = tx_tap<FILTER, BOUNDARY>(z, s, layers, uv, tap);
#pragma unroll
        for (int k = 0; k < NIDX; k++) s_idx[k][tid] = ok ? tap.idx[k] : -1;
        s_fx[tid] = ok ? tap.fx : 0.0f; s_fy[tid] = ok ? tap.fy : 0.0f;
        s_view[tid] = z.view_textures ? (int)(s / z.per_view) : 0;
    }
    __syncthreads();
    constexpr int V = VEC4 ? 4 : 1;
    const int C = z.C, CV = C / V, total = nslots * CV;                      // lane -> (slot, group of V channels), group fastest
    const int dq = TX_BLOCK / CV, dr = TX_BLOCK - dq * CV;                    // the step of (slot, group) per sweep
    int slot = tid / CV, c = tid - slot * CV;
    float* o = out + s0 * C;
    for (int e = tid; e < total; e += TX_BLOCK) {
        const int i00 = s_idx[0][slot];
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};                                // (the scalar path uses r[0] alone)
        if (i00 >= 0) {
            const float* base = tex + (int64_t)s_view[slot] * z.texels * C + (int64_t)c * V;
            if (FILTER == TX_NEAREST) {
                if (VEC4) {
                    const float4 t = *reinterpret_cast<const float4*>(base + (int64_t)i00 * C);
                    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
                } else {
                    r[0] = base[(int64_t)i00 * C];
                }
            } else {
                const float fx = s_fx[slot], fy = s_fy[slot];
                const float* p00 = base + (int64_t)i00 * C;
                const float* p10 = base + (int64_t)s_idx[NIDX > 1 ? 1 : 0][slot] * C;
                const float* p01 = base + (int64_t)s_idx[NIDX > 1 ? 2 : 0][slot] * C;
                const float* p11 = base + (int64_t)s_idx[NIDX > 1 ? 3 : 0][slot] * C;
                if (VEC4) {
                    const float4 t00 = *reinterpret_cast<const float4*>(p00), t10 = *reinterpret_cast<const float4*>(p10);
                    const float4 t01 = *reinterpret_cast<const float4*>(p01), t11 = *reinterpret_cast<const float4*>(p11);
                    r[0] = tx_bilinear(t00.x, t10.x, t01.x, t11.x, fx, fy);
                    r[1] = tx_bilinear(t00.y, t10.y, t01.y, t11.y, fx, fy);
                    r[2] = tx_bilinear(t00.z, t10.z, t01.z, t11.z, fx, fy);
                    r[3] = tx_bilinear(t00.w, t10.w, t01.w, t11.w, fx, fy);
                } else {
                    r[0] = tx_bilinear(*p00, *p10, *p01, *p11, fx, fy);
                }
            }
        }
        if (VEC4) reinterpret_cast<float4*>(o)[e] = make_float4(r[0], r[1], r[2], r[3]);
        else o[e] = r[0];
        slot += dq; c += dr;
        if (c >= CV) { c -= CV; slot++; }
    }
}

// one channel's terms of the two sums
__device__ __forceinline__ void tx_uv_term(float t00, float t10, float t01, float t11, float g, float fx, float fy, float& su, float& sv) {
    const float d0 = t10 - t00, d1 = t11 - t01;
    const float a = t00 + fx * d0, b = t01 + fx * d1;
    su += g * (d0 + fy * (d1 - d0));
    sv += g * (b - a);
}

// (linear only: the entry point zero-fills dL_duv for nearest.)  VEC4 as in k_texture: the sums run over the channels in the
// same order either way.
template <int BOUNDARY, bool VEC4>
__global__ void __launch_bounds__(TX_BLOCK)
k_texture_bwd_uv(TexSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ tex,
                 const float* __restrict__ g, float* __restrict__ dL_duv) {
    const int64_t s = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (s >= z.S) return;
    TexTap tap;
    float su = 0.0f, sv = 0.0f;
    if (tx_tap<TX_LINEAR, BOUNDARY>(z, s, layers, uv, tap)) {
        const int C = z.C;
        const float* base = tex + (z.view_textures ? (s / z.per_view) * z.texels * C : 0);
        const float* p00 = base + (int64_t)tap.idx[0] * C;
        const float* p10 = base + (int64_t)tap.idx[1] * C;
        const float* p01 = base + (int64_t)tap.idx[2] * C;
        const float* p11 = base + (int64_t)tap.idx[3] * C;
        const float* gs = g + s * C;
        if (VEC4) {
            for (int c = 0; c < C; c += 4) {
                const float4 t00 = *reinterpret_cast<const float4*>(p00 + c), t10 = *reinterpret_cast<const float4*>(p10 + c);
                const float4 t01 = *reinterpret_cast<const float4*>(p01 + c), t11 = *reinterpret_cast<const float4*>(p11 + c);
                const float4 gv = *reinterpret_cast<const float4*>(gs + c);
                tx_uv_term(t00.x, t10.x, t01.x, t11.x, gv.x, tap.fx, tap.fy, su, sv);
                tx_uv_term(t00.y, t10.y, t01.y, t11.y, gv.y, tap.fx, tap.fy, su, sv);
                tx_uv_term(t00.z, t10.z, t01.z, t11.z, gv.z, tap.fx, tap.fy, su, sv);
                tx_uv_term(t00.w, t10.w, t01.w, t11.w, gv.w, tap.fx, tap.fy, su, sv);
            }
        } else {
            for (int c = 0; c < C; c++) tx_uv_term(p00[c], p10[c], p01[c], p11[c], gs[c], tap.fx, tap.fy, su, sv);
        }
        su = (float)z.Wt * su; sv = (float)z.Ht * sv;
    }
    dL_duv[2 * s] = su; dL_duv[2 * s + 1] = sv;
}

template <int FILTER, int BOUNDARY, int CH>
__global__ void __launch_bounds__(TILE_PIX)
k_texture_bwd_tex(TexSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ g,
                  float* __restrict__ dL_dtex) {
    constexpr int NTAP = FILTER == TX_LINEAR ? 4 : 1;
    constexpr int STRIDE = LC_SLOTS + (64 + CH - 1) / CH;                     // flush: bank = (c * (64 / CH) + slot) % 64
    __shared__ FaceTable<float, CH, STRIDE> tab;
    const int b = blockIdx.z, tid = threadIdx.x;
    const TilePixel t = tile_pixel(tid, z.W, z.H);
    const int C = z.C, L = z.L;
    float* dst = dL_dtex + (z.view_textures ? (int64_t)b * z.texels * C : 0);
    for (int l = 0; l < L; l++) {
        const int64_t s = t.pix * L + l;
        TexTap tap = {{0, 0, 0, 0}, 0.0f, 0.0f};
        const bool live = t.inside && tx_tap<FILTER, BOUNDARY>(z, s, layers, uv, tap);
        const float w[4] = {(1.0f - tap.fx) * (1.0f - tap.fy), tap.fx * (1.0f - tap.fy), (1.0f - tap.fx) * tap.fy, tap.fx * tap.fy};
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
                for (int k = 0; k < NTAP; k++) {
                    const int key = tap.idx[k];
                    const float wk = FILTER == TX_LINEAR ? w[k] : 1.0f;
                    const int slot = tab.slot(key);
#pragma unroll
                    for (int c = 0; c < CH; c++) {
                        if (c >= nc) continue;
                        const float v = wk * gv[c];
                        if (slot >= 0) tab.add(slot, c, v);
                        else atomicAdd(dst + (int64_t)key * C + c0 + c, v);
                    }
                }
            }
            __syncthreads();
            // flush: one global atomic per (texel, channel) the table holds; lane -> (slot, c), c fastest
            tab.flush_by_slot(tid, [&](int key, int c, float v) {
                if (c < nc) atomicAdd(dst + (int64_t)key * C + c0 + c, v);
            });
            __syncthreads();
        }
    }
}

static TexSizes tx_sizes(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures) {
    TexSizes z;
    z.per_view = (int64_t)H * W * L;
    z.S = (int64_t)B * z.per_view;
    z.texels = (int64_t)Ht * Wt;
    z.B = B; z.H = H; z.W = W; z.L = L; z.Ht = Ht; z.Wt = Wt; z.C = C; z.view_textures = view_textures;
    return z;
}

static bool tx_aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

// X(F, Bd) with the call's runtime (filter, boundary) as compile-time constants
#define DM2_TX_MODES(filter, boundary, X)                                  \
    do {                                                                   \
        if ((filter) == TX_LINEAR) {                                       \
            if ((boundary) == TX_WRAP) { X(TX_LINEAR, TX_WRAP); } else { X(TX_LINEAR, TX_CLAMP); }   \
        } else {                                                           \
            if ((boundary) == TX_WRAP) { X(TX_NEAREST, TX_WRAP); } else { X(TX_NEAREST, TX_CLAMP); } \
        }                                                                  \
    } while (0)

void launch_texture(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures, int filter, int boundary,
                    const int32_t* render_layers, const float* uv, const float* tex, float* out, hipStream_t st) {
    const TexSizes z = tx_sizes(B, H, W, L, Ht, Wt, C, view_textures);
    const dim3 grid((unsigned)((z.S + TX_BLOCK - 1) / TX_BLOCK));
    const bool vec4 = C % 4 == 0 && tx_aligned16(tex, out);
#define DM2_TX_FWD(F, Bd)                                                                                                       \
    if (vec4) hipLaunchKernelGGL((k_texture<F, Bd, true>), grid, dim3(TX_BLOCK), 0, st, z, render_layers, uv, tex, out);       \
    else hipLaunchKernelGGL((k_texture<F, Bd, false>), grid, dim3(TX_BLOCK), 0, st, z, render_layers, uv, tex, out)
    DM2_TX_MODES(filter, boundary, DM2_TX_FWD);
#undef DM2_TX_FWD
}

void launch_texture_backward(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures, int filter, int boundary,
                             const int32_t* render_layers, const float* uv, const float* tex, const float* dL_dout,
                             float* dL_dtex, float* dL_duv, hipStream_t st) {
    const TexSizes z = tx_sizes(B, H, W, L, Ht, Wt, C, view_textures);
    if (dL_duv) {
        const dim3 grid((unsigned)((z.S + TX_BLOCK - 1) / TX_BLOCK));       // (linear: the entry point zero-fills for nearest)
        const bool vec4 = C % 4 == 0 && tx_aligned16(tex, dL_dout);
#define DM2_TX_UV(Bd, V4) hipLaunchKernelGGL((k_texture_bwd_uv<Bd, V4>), grid, dim3(TX_BLOCK), 0, st, z, render_layers, uv, tex, dL_dout, dL_duv)
        if (boundary == TX_WRAP) { if (vec4) DM2_TX_UV(TX_WRAP, true); else DM2_TX_UV(TX_WRAP, false); }
        else { if (vec4) DM2_TX_UV(TX_CLAMP, true); else DM2_TX_UV(TX_CLAMP, false); }
#undef DM2_TX_UV
    }
    if (dL_dtex) {
        const dim3 grid = tile_grid(W, H, B);
#define DM2_TX_TEX_CH(F, Bd, CH) hipLaunchKernelGGL((k_texture_bwd_tex<F, Bd, CH>), grid, dim3(TILE_PIX), 0, st, z, render_layers, uv, dL_dout, dL_dtex)
#define DM2_TX_TEX(F, Bd)                       \
    if (C == 1) DM2_TX_TEX_CH(F, Bd, 1);        \
    else if (C == 2) DM2_TX_TEX_CH(F, Bd, 2);   \
    else if (C == 3) DM2_TX_TEX_CH(F, Bd, 3);   \
    else DM2_TX_TEX_CH(F, Bd, TX_CH)
        DM2_TX_MODES(filter, boundary, DM2_TX_TEX);
#undef DM2_TX_TEX
#undef DM2_TX_TEX_CH
    }
}

#undef DM2_TX_MODES

}  // namespace dm2
