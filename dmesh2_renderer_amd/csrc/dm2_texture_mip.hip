// dm2_texture_mip.hip -- Renderer.texture_mipmaps and Renderer.texture(filter_mode="linear-mipmap-linear"):
//   k_mip_level          level k+1 of the chain from level k: ((p00 + p10) + (p01 + p11)) * 0.25f over the 2 x 2 parents
//   k_mip_backward       dL/dtex[j, i] = sum_{k >= 1} 0.25^k dL/dmip_k[j >> k, i >> k]: a gather, no atomics
//   k_texture_mip        out[s, c] = c_j + f (c_{j+1} - c_j), c_k = the bilinear sample of level k (one level where lod <= 0 or
//                        lod >= nlev - 1)
//   k_texture_mip_bwd_uv dL/duv[s] = (1 - f) duv_j + f duv_{j+1}
//   k_texture_mip_bwd_tex  dL/dtex, dL/dmip[t_pq of level j, j+1] += (1 - f) w_pq g, f w_pq g
//
// Contract: include/dm2_hip.h, dm2_texture_mipmaps / dm2_texture_mip.  The level of detail comes from the float's bits (log2
// with the mantissa taken linearly: no transcendental), so the forward is a pure function of IEEE operations.
// -ffp-contract=off: the written operation order is the result.  The sampling of one level is dm2_texture's: both take it from
// dm2_tex_core.h (the taps and fractions of one level, the blend, the uv terms, the sweep, the scatter).
//
// A texel of any level has one index in a single space: level 0's j * Wt + i first, then the packed chain (texels + off_k +
// j * W_k + i).  The forward stages those indices, the scatter keys its LDS table by them.
//
// Forward: the kernel of dm2_texture.hip with twice the taps: flat slots, 256 per block, each lane stages its slot's eight
// indices, the fractions of the two levels and f in LDS, then the block sweeps its 256 * C outputs with consecutive lanes on
// consecutive channels (four per lane on the vector path).
// tex backward: k_texture_bwd_tex's tile scatter (tex_scatter_layer: one block per 16 x 16 tile and view, one layer at a time,
// channel chunks of CH, the FaceTable cleared per layer) with up to eight (texel, weight) pairs per slot; the two gradient
// tensors, either of which may be absent, are behind the one key space.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"
#include "dm2_tex_core.h"

namespace dm2 {

constexpr int TM_MAX_LEVELS = 16;                     // Ht * Wt < 2^31 with both extents even at every step: at most 16 levels

struct MipSizes {
    int64_t S, per_view;
    int64_t texels;   // Ht * Wt
    int64_t T;        // texels of the packed chain (levels 1 .. nlev - 1); texels + T < 2^31
    int B, H, W, L, Ht, Wt, C, view_textures, nlev;
};

// one slot's sample: per level (j, j + 1) the single-space indices of t00, t10, t01, t11 and the fractions; f < 0: one level
struct MipTap {
    int idx[2][4];
    float fx[2], fy[2];
    float f;
    int j;            // the level of idx[0] (idx[1]: j + 1)
};

// s_off[k], k >= 1: the first texel of level k in the packed chain
__device__ __forceinline__ void tm_offsets(const MipSizes& z, int* s_off, int tid) {
    if (tid < TM_MAX_LEVELS) {
        int o = 0;
        for (int i = 1; i < tid; i++) o += (z.Ht >> i) * (z.Wt >> i);
        s_off[tid] = o;
    }
}

// level k's taps at (u, v): dm2_texture's linear stage with that level's extents (W_k = Wt >> k: every step halved an even extent)
template <int BOUNDARY>
__device__ __forceinline__ void tm_level(const MipSizes& z, const int* s_off, int k, float u, float v, int (&idx)[4], float& fx, float& fy) {
    const int Wk = z.Wt >> k, Hk = z.Ht >> k;
    const float x = u * (float)Wk - 0.5f, y = v * (float)Hk - 0.5f;
    tex_linear_taps<BOUNDARY>(Wk, Hk, k == 0 ? 0 : (int)z.texels + s_off[k], x, y, idx, fx, fy);
}

__device__ __forceinline__ bool tm_finite(float a) { return fabsf(a) < __builtin_inff(); }

// false = empty slot (nothing of ``tap`` is set)
template <int BOUNDARY>
__device__ __forceinline__ bool tm_tap(const MipSizes& z, const int* s_off, int64_t s, const int32_t* __restrict__ layers,
                                       const float* __restrict__ uv, const float* __restrict__ uv_da, MipTap& tap) {
    if (layers && layers[s] < 0) return false;
    const float u = uv[2 * s], v = uv[2 * s + 1];
    const float x = u * (float)z.Wt - 0.5f, y = v * (float)z.Ht - 0.5f;
    if (!(fabsf(x) < TEX_RANGE) || !(fabsf(y) < TEX_RANGE)) return false;          // level 0's rule: NaN and infinities included
    const float dudx = uv_da[4 * s], dvdx = uv_da[4 * s + 1], dudy = uv_da[4 * s + 2], dvdy = uv_da[4 * s + 3];
    if (!(tm_finite(dudx) && tm_finite(dvdx) && tm_finite(dudy) && tm_finite(dvdy))) return false;
    const float ax = dudx * (float)z.Wt, bx = dvdx * (float)z.Ht, sx = ax * ax + bx * bx;
    const float ay = dudy * (float)z.Wt, by = dvdy * (float)z.Ht, sy = ay * ay + by * by;
    const float r2 = fmaxf(sx, sy);
    float lod = 0.0f;
    if (r2 > 1.0f) {                                                             // r2 = m 2^e, m in [1, 2)
        const uint32_t bits = __float_as_uint(r2);
        const int e = (int)(bits >> 23) - 127;
        const float m = __uint_as_float((bits & 0x007FFFFFu) | 0x3F800000u);
        lod = 0.5f * ((float)e + (m - 1.0f));
    }
    int j;
    if (lod <= 0.0f) { j = 0; tap.f = -1.0f; }
    else if (lod >= (float)(z.nlev - 1)) { j = z.nlev - 1; tap.f = -1.0f; }
    else { j = (int)floorf(lod); tap.f = lod - (float)j; }
    tap.j = j;
    tm_level<BOUNDARY>(z, s_off, j, u, v, tap.idx[0], tap.fx[0], tap.fy[0]);
    if (tap.f >= 0.0f) {
        tm_level<BOUNDARY>(z, s_off, j + 1, u, v, tap.idx[1], tap.fx[1], tap.fy[1]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) tap.idx[1][k] = tap.idx[0][k];
        tap.fx[1] = tap.fx[0]; tap.fy[1] = tap.fy[0];
    }
    return true;
}

// the row of single-space texel ``key``: level 0 in tex, the rest in the chain (texv, mipv: the view's own where per view)
__device__ __forceinline__ const float* tm_row(const MipSizes& z, const float* texv, const float* mipv, int key) {
    return key < (int)z.texels ? texv + (int64_t)key * z.C : mipv + ((int64_t)key - z.texels) * z.C;
}

template <bool VEC4>
__device__ __forceinline__ void tm_sample(const MipSizes& z, const float* texv, const float* mipv, int i00, int i10, int i01, int i11,
                                          int c, float fx, float fy, float (&r)[4]) {
    const TexQuad q = tex_sample_rows<VEC4>(tm_row(z, texv, mipv, i00) + c, tm_row(z, texv, mipv, i10) + c, tm_row(z, texv, mipv, i01) + c,
                                            tm_row(z, texv, mipv, i11) + c, fx, fy);
    r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w;
}

// VEC4: C is a multiple of 4 and tex / mip / out are 16-byte aligned; every channel goes through the same operations either way.
template <int BOUNDARY, bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_mip(MipSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ uv_da,
              const float* __restrict__ tex, const float* __restrict__ mip, float* __restrict__ out) {
    __shared__ int s_idx[8][TEX_BLOCK];                                        // s_idx[0] < 0: empty slot
    __shared__ float s_fx[2][TEX_BLOCK], s_fy[2][TEX_BLOCK], s_f[TEX_BLOCK];
    __shared__ int s_view[TEX_BLOCK];
    __shared__ int s_off[TM_MAX_LEVELS];
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * TEX_BLOCK;
    const int nslots = (int)min((int64_t)TEX_BLOCK, z.S - s0);
    tm_offsets(z, s_off, tid);
    __syncthreads();
    if (tid < nslots) {
        const int64_t s = s0 + tid;
        MipTap tap;
        const bool ok = tm_tap<BOUNDARY>(z, s_off, s, layers, uv, uv_da, tap);
#pragma unroll
        for (int l = 0; l < 2; l++) {
#pragma unroll
            for (int k = 0; k < 4; k++) s_idx[4 * l + k][tid] = ok ? tap.idx[l][k] : -1;
            s_fx[l][tid] = ok ? tap.fx[l] : 0.0f; s_fy[l][tid] = ok ? tap.fy[l] : 0.0f;
        }
        s_f[tid] = ok ? tap.f : -1.0f;
        s_view[tid] = z.view_textures ? (int)(s / z.per_view) : 0;
    }
    __syncthreads();
    // (tex_sweep's loop, written out: through tex_sweep the two view offsets compile to other instructions than they were)
    constexpr int V = VEC4 ? 4 : 1;
    const int C = z.C, CV = C / V, total = nslots * CV;                      // lane -> (slot, group of V channels), group fastest
    const int dq = TEX_BLOCK / CV, dr = TEX_BLOCK - dq * CV;
    int slot = tid / CV, c = tid - slot * CV;
    float* o = out + s0 * C;
    for (int e = tid; e < total; e += TEX_BLOCK) {
        const int i00 = s_idx[0][slot];
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i00 >= 0) {
            const float* texv = tex + (int64_t)s_view[slot] * z.texels * C;
            const float* mipv = mip + (int64_t)s_view[slot] * z.T * C;
            const float f = s_f[slot];
            tm_sample<VEC4>(z, texv, mipv, i00, s_idx[1][slot], s_idx[2][slot], s_idx[3][slot], c * V, s_fx[0][slot], s_fy[0][slot], r);
            if (f >= 0.0f) {
                float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                tm_sample<VEC4>(z, texv, mipv, s_idx[4][slot], s_idx[5][slot], s_idx[6][slot], s_idx[7][slot], c * V, s_fx[1][slot],
                                s_fy[1][slot], q);
#pragma unroll
                for (int k = 0; k < V; k++) r[k] = r[k] + f * (q[k] - r[k]);
            }
        }
        if (VEC4) reinterpret_cast<float4*>(o)[e] = make_float4(r[0], r[1], r[2], r[3]);
        else o[e] = r[0];
        slot += dq; c += dr;
        if (c >= CV) { c -= CV; slot++; }
    }
}

// one level's (sum_c g d/dx, sum_c g d/dy) in texel units, the channels in order
__device__ __forceinline__ void tm_uv_level(const MipSizes& z, const float* texv, const float* mipv, const int (&idx)[4], float fx, float fy,
                                            const float* __restrict__ gs, float& su, float& sv) {
    const float* p00 = tm_row(z, texv, mipv, idx[0]);
    const float* p10 = tm_row(z, texv, mipv, idx[1]);
    const float* p01 = tm_row(z, texv, mipv, idx[2]);
    const float* p11 = tm_row(z, texv, mipv, idx[3]);
    su = 0.0f; sv = 0.0f;
    for (int c = 0; c < z.C; c++) tex_uv_term(p00[c], p10[c], p01[c], p11[c], gs[c], fx, fy, su, sv);
}

template <int BOUNDARY>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_mip_bwd_uv(MipSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ uv_da,
                     const float* __restrict__ tex, const float* __restrict__ mip, const float* __restrict__ g,
                     float* __restrict__ dL_duv) {
    __shared__ int s_off[TM_MAX_LEVELS];
    tm_offsets(z, s_off, threadIdx.x);
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (s >= z.S) return;
    MipTap tap;
    float du = 0.0f, dv = 0.0f;
    if (tm_tap<BOUNDARY>(z, s_off, s, layers, uv, uv_da, tap)) {
        const int C = z.C;
        const int64_t view = z.view_textures ? s / z.per_view : 0;
        const float* texv = tex + view * z.texels * C;
        const float* mipv = mip + view * z.T * C;
        const float* gs = g + s * C;
        float su, sv;
        tm_uv_level(z, texv, mipv, tap.idx[0], tap.fx[0], tap.fy[0], gs, su, sv);
        const int j = tap.j;
        const float Wj = (float)(z.Wt >> j), Hj = (float)(z.Ht >> j);
        du = Wj * su; dv = Hj * sv;
        if (tap.f >= 0.0f) {
            float su1, sv1;
            tm_uv_level(z, texv, mipv, tap.idx[1], tap.fx[1], tap.fy[1], gs, su1, sv1);
            const float W1 = (float)(z.Wt >> (j + 1)), H1 = (float)(z.Ht >> (j + 1));
            du = (1.0f - tap.f) * du + tap.f * (W1 * su1);
            dv = (1.0f - tap.f) * dv + tap.f * (H1 * sv1);
        }
    }
    dL_duv[2 * s] = du; dL_duv[2 * s + 1] = dv;
}

template <int BOUNDARY, int CH>
__global__ void __launch_bounds__(TILE_PIX)
k_texture_mip_bwd_tex(MipSizes z, const int32_t* __restrict__ layers, const float* __restrict__ uv, const float* __restrict__ uv_da,
                      const float* __restrict__ g, float* __restrict__ dL_dtex, float* __restrict__ dL_dmip) {
    __shared__ TexTable<CH> tab;
    __shared__ int s_off[TM_MAX_LEVELS];
    const int b = blockIdx.z, tid = threadIdx.x;
    const TilePixel t = tile_pixel(tid, z.W, z.H);
    const int C = z.C, L = z.L;
    const int texels = (int)z.texels;
    // either may be null (not wanted): its texels are skipped
    float* dtex = dL_dtex ? dL_dtex + (z.view_textures ? (int64_t)b * z.texels * C : 0) : nullptr;
    float* dmip = dL_dmip ? dL_dmip + (z.view_textures ? (int64_t)b * z.T * C : 0) : nullptr;
    // the row of single-space texel ``key`` in its gradient, null where that gradient is not wanted
    auto row = [&](int key) -> float* {
        if (key < texels) return dtex ? dtex + (int64_t)key * C : nullptr;
        return dmip ? dmip + (int64_t)(key - texels) * C : nullptr;
    };
    tm_offsets(z, s_off, tid);
    __syncthreads();
    for (int l = 0; l < L; l++) {
        const int64_t s = t.pix * L + l;
        MipTap tap = {{{0, 0, 0, 0}, {0, 0, 0, 0}}, {0.0f, 0.0f}, {0.0f, 0.0f}, -1.0f, 0};
        const bool live = t.inside && tm_tap<BOUNDARY>(z, s_off, s, layers, uv, uv_da, tap);
        const bool two = tap.f >= 0.0f;
        const float wl[2] = {two ? 1.0f - tap.f : 1.0f, two ? tap.f : 0.0f};
        float w[2][4];
#pragma unroll
        for (int lv = 0; lv < 2; lv++) {
            const float fx = tap.fx[lv], fy = tap.fy[lv];
            w[lv][0] = wl[lv] * ((1.0f - fx) * (1.0f - fy)); w[lv][1] = wl[lv] * (fx * (1.0f - fy));
            w[lv][2] = wl[lv] * ((1.0f - fx) * fy); w[lv][3] = wl[lv] * (fx * fy);
        }
        // (the eight pairs as flat lists: tap.idx and w are [2][4], level j's four first)
        tex_scatter_layer<CH, 8, true>(tab, tid, live, &tap.idx[0][0], &w[0][0], two ? 8 : 4, -1, g, s, C, row);
    }
}

// level k+1 from level k of every texture: lane -> (texel, channel), channel fastest; the view on blockIdx.y
__global__ void __launch_bounds__(TEX_BLOCK)
k_mip_level(int64_t n /* H1 * W1 * C */, int W1, int C, const float* __restrict__ src, int64_t src_stride, float* __restrict__ dst,
            int64_t dst_stride) {
    const int64_t e = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (e >= n) return;
    const int64_t t = e / C;
    const int c = (int)(e - t * C);
    const int j = (int)(t / W1), i = (int)(t - (int64_t)j * W1);
    const int W0 = 2 * W1;
    const float* p = src + (int64_t)blockIdx.y * src_stride + ((int64_t)(2 * j) * W0 + 2 * i) * C + c;
    const float p00 = p[0], p10 = p[C], p01 = p[(int64_t)W0 * C], p11 = p[(int64_t)W0 * C + C];
    dst[(int64_t)blockIdx.y * dst_stride + e] = ((p00 + p10) + (p01 + p11)) * 0.25f;
}

// lane -> (texel of level 0, channel); acc = acc + 0.25^k g_k over the levels in order
__global__ void __launch_bounds__(TEX_BLOCK)
k_mip_backward(int64_t n /* Ht * Wt * C */, int Ht, int Wt, int C, int nlev, int64_t T, const float* __restrict__ dL_dmip,
               float* __restrict__ dL_dtex) {
    const int64_t e = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (e >= n) return;
    const int64_t t = e / C;
    const int c = (int)(e - t * C);
    const int j = (int)(t / Wt), i = (int)(t - (int64_t)j * Wt);
    const float* gm = dL_dmip + (int64_t)blockIdx.y * T * C;
    float acc = 0.0f, wk = 1.0f;
    int64_t off = 0;
    for (int k = 1; k < nlev; k++) {
        const int Wk = Wt >> k, Hk = Ht >> k;
        wk = wk * 0.25f;
        acc = acc + wk * gm[(off + (int64_t)(j >> k) * Wk + (i >> k)) * C + c];
        off += (int64_t)Wk * Hk;
    }
    dL_dtex[(int64_t)blockIdx.y * n + e] = acc;
}

// 1 + the levels built; *T: the chain's texels (levels 1 .. nlev - 1).  max_level < 0: no limit.
int mip_levels(int Ht, int Wt, int max_level, int64_t* T) {
    int nlev = 1, h = Ht, w = Wt;
    int64_t total = 0;
    while (h % 2 == 0 && w % 2 == 0 && (max_level < 0 || nlev - 1 < max_level)) {
        h /= 2; w /= 2;
        total += (int64_t)h * w;
        nlev++;
    }
    if (T) *T = total;
    return nlev;
}

static MipSizes tm_sizes(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures, int max_level) {
    MipSizes z;
    tex_common_sizes(z, B, H, W, L, C, view_textures);
    z.texels = (int64_t)Ht * Wt;
    z.nlev = mip_levels(Ht, Wt, max_level, &z.T);
    z.Ht = Ht; z.Wt = Wt;
    return z;
}

void launch_texture_mipmaps(int NB, int Ht, int Wt, int C, int max_level, const float* tex, float* mip, hipStream_t st) {
    int64_t T;
    const int nlev = mip_levels(Ht, Wt, max_level, &T);
    const float* src = tex;
    int64_t src_stride = (int64_t)Ht * Wt * C, off = 0;
    for (int k = 1; k < nlev; k++) {
        const int W1 = Wt >> k, H1 = Ht >> k;
        const int64_t n = (int64_t)H1 * W1 * C;
        float* dst = mip + off * C;
        hipLaunchKernelGGL(k_mip_level, tex_flat_grid(n, NB), dim3(TEX_BLOCK), 0, st, n, W1, C, src, src_stride, dst, T * C);
        src = dst; src_stride = T * C;
        off += (int64_t)H1 * W1;
    }
}

void launch_texture_mipmaps_backward(int NB, int Ht, int Wt, int C, int max_level, const float* dL_dmip, float* dL_dtex, hipStream_t st) {
    int64_t T;
    const int nlev = mip_levels(Ht, Wt, max_level, &T);
    const int64_t n = (int64_t)Ht * Wt * C;
    hipLaunchKernelGGL(k_mip_backward, tex_flat_grid(n, NB), dim3(TEX_BLOCK), 0, st, n, Ht, Wt, C, nlev, T, dL_dmip, dL_dtex);
}

void launch_texture_mip(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures, int boundary, int max_level,
                        const int32_t* render_layers, const float* uv, const float* uv_da, const float* tex, const float* mip,
                        float* out, hipStream_t st) {
    const MipSizes z = tm_sizes(B, H, W, L, Ht, Wt, C, view_textures, max_level);
    const dim3 grid = tex_flat_grid(z.S);
    const bool vec4 = C % 4 == 0 && tex_aligned16(tex, out, mip);
#define DM2_TM_FWD(Bd, V4) hipLaunchKernelGGL((k_texture_mip<Bd, V4>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, uv, uv_da, tex, mip, out)
    if (boundary == TEX_WRAP) { if (vec4) DM2_TM_FWD(TEX_WRAP, true); else DM2_TM_FWD(TEX_WRAP, false); }
    else { if (vec4) DM2_TM_FWD(TEX_CLAMP, true); else DM2_TM_FWD(TEX_CLAMP, false); }
#undef DM2_TM_FWD
}

void launch_texture_mip_backward(int B, int H, int W, int L, int Ht, int Wt, int C, int view_textures, int boundary, int max_level,
                                 const int32_t* render_layers, const float* uv, const float* uv_da, const float* tex,
                                 const float* mip, const float* dL_dout, float* dL_dtex, float* dL_dmip, float* dL_duv,
                                 hipStream_t st) {
    const MipSizes z = tm_sizes(B, H, W, L, Ht, Wt, C, view_textures, max_level);
    if (dL_duv) {
        const dim3 grid = tex_flat_grid(z.S);
#define DM2_TM_UV(Bd) hipLaunchKernelGGL((k_texture_mip_bwd_uv<Bd>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, uv, uv_da, tex, mip, dL_dout, dL_duv)
        if (boundary == TEX_WRAP) DM2_TM_UV(TEX_WRAP); else DM2_TM_UV(TEX_CLAMP);
#undef DM2_TM_UV
    }
    if (dL_dtex || dL_dmip) {
        const dim3 grid = tile_grid(W, H, B);
#define DM2_TM_TEX(Bd, CH) hipLaunchKernelGGL((k_texture_mip_bwd_tex<Bd, CH>), grid, dim3(TILE_PIX), 0, st, z, render_layers, uv, uv_da, dL_dout, dL_dtex, dL_dmip)
        if (boundary == TEX_WRAP) DM2_TEX_CHUNK(C, DM2_TM_TEX, TEX_WRAP); else DM2_TEX_CHUNK(C, DM2_TM_TEX, TEX_CLAMP);
#undef DM2_TM_TEX
    }
}

}  // namespace dm2
