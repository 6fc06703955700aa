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
// tex backward: the tile scatter that dm2_tex_core.h describes at tex_scatter_layer() (the mip and the cube op run it through
// that function; here its body is written out, see k_texture_bwd_tex), keyed by the texel's linear index j * Wt + i, four
// (texel, weight) pairs per slot (nearest: one, weight 1).
// The addressing, the blend and the sweep are dm2_tex_core.h's, shared with the mip and the cube op.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"
#include "dm2_tex_core.h"

namespace dm2 {

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

// false = empty slot (nothing of ``tap`` is set)
template <int FILTER, int BOUNDARY>
__device__ __forceinline__ bool tx_tap(const TexSizes& z, int64_t s, const int32_t* __restrict__ layers,
                                       const float* __restrict__ uv, TexTap& tap) {
    if (layers && layers[s] < 0) return false;
    const float u = uv[2 * s], v = uv[2 * s + 1];
    const float x = u * (float)z.Wt - 0.5f, y = v * (float)z.Ht - 0.5f;
    if (!(fabsf(x) < TEX_RANGE) || !(fabsf(y) < TEX_RANGE)) return false;          // NaN and infinities included
    if (FILTER == TEX_NEAREST) {
        const int i = tex_addr<BOUNDARY>((int)floorf(x + 0.5f), z.Wt), j = tex_addr<BOUNDARY>((int)floorf(y + 0.5f), z.Ht);
        tap.idx[0] = j * z.Wt + i;
        tap.idx[1] = tap.idx[2] = tap.idx[3] = tap.idx[0];
        tap.fx = tap.fy = 0.0f;
        return true;
    }
    tex_linear_taps<BOUNDARY>(z.Wt, z.Ht, 0, x, y, tap.idx, tap.fx, tap.fy);
    return true;
}

template <int FILTER, int BOUNDARY, bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture(TexSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ tex,
          float* __restrict__ out) {
    constexpr int NIDX = FILTER == TEX_LINEAR ? 4 : 1;
    __shared__ int s_idx[NIDX][TEX_BLOCK];                                    // idx[0] < 0: empty slot
    __shared__ float s_fx[TEX_BLOCK], s_fy[TEX_BLOCK];
    __shared__ int s_view[TEX_BLOCK];
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * TEX_BLOCK;
    const int nslots = (int)min((int64_t)TEX_BLOCK, z.S - s0);
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
    const int C = z.C;
    tex_sweep<VEC4>(tid, nslots, C, s_idx[0], out, s0, [&](int slot, int i00, int c) -> TexQuad {
        const float* base = tex + (int64_t)s_view[slot] * z.texels * C + (int64_t)c * (VEC4 ? 4 : 1);
        if (FILTER == TEX_NEAREST) return tex_load_row<VEC4>(base + (int64_t)i00 * C);
        const float fx = s_fx[slot], fy = s_fy[slot];
        const float* p00 = base + (int64_t)i00 * C;
        const float* p10 = base + (int64_t)s_idx[NIDX > 1 ? 1 : 0][slot] * C;
        const float* p01 = base + (int64_t)s_idx[NIDX > 1 ? 2 : 0][slot] * C;
        const float* p11 = base + (int64_t)s_idx[NIDX > 1 ? 3 : 0][slot] * C;
        return tex_sample_rows<VEC4>(p00, p10, p01, p11, fx, fy);
    });
}

// (linear only: the entry point zero-fills dL_duv for nearest.)  The sums run over the channels in the same order on the
// VEC4 path.
template <int BOUNDARY, bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_bwd_uv(TexSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ tex,
                 const float* __restrict__ g, float* __restrict__ dL_duv) {
    const int64_t s = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (s >= z.S) return;
    TexTap tap;
    float su = 0.0f, sv = 0.0f;
    if (tx_tap<TEX_LINEAR, BOUNDARY>(z, s, layers, uv, tap)) {
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
                tex_uv_term(t00.x, t10.x, t01.x, t11.x, gv.x, tap.fx, tap.fy, su, sv);
                tex_uv_term(t00.y, t10.y, t01.y, t11.y, gv.y, tap.fx, tap.fy, su, sv);
                tex_uv_term(t00.z, t10.z, t01.z, t11.z, gv.z, tap.fx, tap.fy, su, sv);
                tex_uv_term(t00.w, t10.w, t01.w, t11.w, gv.w, tap.fx, tap.fy, su, sv);
            }
        } else {
            for (int c = 0; c < C; c++) tex_uv_term(p00[c], p10[c], p01[c], p11[c], gs[c], tap.fx, tap.fy, su, sv);
        }
        su = (float)z.Wt * su; sv = (float)z.Ht * sv;
    }
    dL_duv[2 * s] = su; dL_duv[2 * s + 1] = sv;
}

template <int FILTER, int BOUNDARY, int CH>
__global__ void __launch_bounds__(TILE_PIX)
k_texture_bwd_tex(TexSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ g,
                  float* __restrict__ dL_dtex) {
    constexpr int NTAP = FILTER == TEX_LINEAR ? 4 : 1;
    __shared__ TexTable<CH> tab;
    const int b = blockIdx.z, tid = threadIdx.x;
    const TilePixel t = tile_pixel(tid, z.W, z.H);
    const int C = z.C, L = z.L;
    float* dst = dL_dtex + (z.view_textures ? (int64_t)b * z.texels * C : 0);
    for (int l = 0; l < L; l++) {
        const int64_t s = t.pix * L + l;
        TexTap tap = {{0, 0, 0, 0}, 0.0f, 0.0f};
        const bool live = t.inside && tx_tap<FILTER, BOUNDARY>(z, s, layers, uv, tap);
        const float w[4] = {(1.0f - tap.fx) * (1.0f - tap.fy), tap.fx * (1.0f - tap.fy), (1.0f - tap.fx) * tap.fy, tap.fx * tap.fy};
        // tex_scatter_layer's body, written out: through the shared function this kernel's 64-bit row addresses compile to 13
        // instructions more per layer, and <linear, clamp, 4> measured 0.2 % slower, outside its spread (profiles/texture_core_ab.txt)
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
                    const float wk = FILTER == TEX_LINEAR ? w[k] : 1.0f;
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
            tab.flush_by_slot(tid, [&](int key, int c, float v) {
                if (c < nc) atomicAdd(dst + (int64_t)key * C + c0 + c, v);
            });
            __syncthreads();
        }
    }
}

static TexSizes tx_sizes(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures) {
    TexSizes z;
    tex_common_sizes(z, B, H, W, L, C, view_textures);
    z.texels = (int64_t)Ht * Wt;
    z.Ht = Ht; z.Wt = Wt;
    return z;
}

void launch_texture(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures, int filter, int boundary,
                    const int32_t* render_layers, const float* uv, const float* tex, float* out, hipStream_t st) {
    const TexSizes z = tx_sizes(B, H, W, L, Ht, Wt, C, view_textures);
    const dim3 grid = tex_flat_grid(z.S);
    const bool vec4 = C % 4 == 0 && tex_aligned16(tex, out);
#define DM2_TX_FWD(F, Bd)                                                                                                       \
    if (vec4) hipLaunchKernelGGL((k_texture<F, Bd, true>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, uv, tex, out);      \
    else hipLaunchKernelGGL((k_texture<F, Bd, false>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, uv, tex, out)
    DM2_TEX_MODES(filter, boundary, DM2_TX_FWD);
#undef DM2_TX_FWD
}

void launch_texture_backward(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures, int filter, int boundary,
                             const int32_t* render_layers, const float* uv, const float* tex, const float* dL_dout,
                             float* dL_dtex, float* dL_duv, hipStream_t st) {
    const TexSizes z = tx_sizes(B, H, W, L, Ht, Wt, C, view_textures);
    if (dL_duv) {
        const dim3 grid = tex_flat_grid(z.S);                               // (linear: the entry point zero-fills for nearest)
        const bool vec4 = C % 4 == 0 && tex_aligned16(tex, dL_dout);
#define DM2_TX_UV(Bd, V4) hipLaunchKernelGGL((k_texture_bwd_uv<Bd, V4>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, uv, tex, dL_dout, dL_duv)
        if (boundary == TEX_WRAP) { if (vec4) DM2_TX_UV(TEX_WRAP, true); else DM2_TX_UV(TEX_WRAP, false); }
        else { if (vec4) DM2_TX_UV(TEX_CLAMP, true); else DM2_TX_UV(TEX_CLAMP, false); }
#undef DM2_TX_UV
    }
    if (dL_dtex) {
        const dim3 grid = tile_grid(W, H, B);
#define DM2_TX_TEX_CH(F, Bd, CH) hipLaunchKernelGGL((k_texture_bwd_tex<F, Bd, CH>), grid, dim3(TILE_PIX), 0, st, z, render_layers, uv, dL_dout, dL_dtex)
#define DM2_TX_TEX(F, Bd) DM2_TEX_CHUNK(C, DM2_TX_TEX_CH, F, Bd)
        DM2_TEX_MODES(filter, boundary, DM2_TX_TEX);
#undef DM2_TX_TEX
#undef DM2_TX_TEX_CH
    }
}

}  // namespace dm2
