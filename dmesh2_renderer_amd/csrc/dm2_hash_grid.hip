// dm2_hash_grid.hip -- Renderer.hash_grid: a multiresolution hash encoding, table (NL, T, F), looked up by a position (x, y, z)
// in the field's unit cube per slot s = (b, y, x, l).  Level v is texture3d's lookup of a virtual R_v^3 grid whose voxel
// (k, j, i) lives in row row_v(k, j, i) of table[v]:
//   k_hash_grid            out[s, v F + f] = a0 + fz (a1 - a0), a_r the bilinear blend of plane k0 + r's four taps (nearest: one row)
//   k_hash_grid_bwd_xyz    dL/dxyz[s] = sum_v R_v (su0 + fz (su1 - su0), sv0 + fz (sv1 - sv0), sum_f g (a1 - a0)), v = 0 .. NL - 1 in
//                          that order, su_r, sv_r the uv terms (tex_uv_term) of plane r over the level's F features
//   k_hash_grid_bwd_table  dL/dtable[v, row_pqr, f] += w_pqr g[s, v F + f]
//
// Contract (include/dm2_hip.h, dm2_hash_grid): X = x R_v - 0.5 in fp32, X0 = floor(X),
// fx = X - X0, Y and Z alike; the taps through dm2_texture's addr with n = R_v; row = (k R_v + j) R_v + i where R_v^3 <= T, else
// (i ^ j 2654435761 ^ k 805459861) mod T in wrapping 32-bit arithmetic, on the addresses after addr.  A slot is empty when its
// id is negative or |X|, |Y| or |Z| at the finest level is not below 2^24 (NaN and infinite coordinates included): zeros in
// every channel, nothing read from the table through it, no gradient.  -ffp-contract=off: the forward is a pure function of the
// written operation order.
//
// The host works the R_v out once per call (HashLevels, by value: 32 ints and a dense / hashed bit per level).
// Forward: one lane per (slot, level), the level on blockIdx.y, so the blocks in flight gather from one level's table (at
// T = 2^19, F = 2 that is 4 MiB, one XCD's L2); a tap's F features are one load of 4 F bytes (F = 8: two of 16), the slot's F
// outputs one store.  Position backward: one lane per slot, the levels in order, plain stores.  Table backward: one block per
// 16 x 16 pixel tile, view and level, one layer at a time through the block's table (tex_scatter_layer_masked) keyed by the row
// index, which is taken after hashing, so two pixels in one voxel merge on a hashed level too; a coarse level merges nearly
// everything in LDS, the finest levels mostly take the table's overflow route straight to global atomics.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"
#include "dm2_tex_core.h"

namespace dm2 {

constexpr int HG_MAX_LEVELS = 32;

struct HashLevels {
    int R[HG_MAX_LEVELS];   // the resolution of level v
    uint32_t dense;         // bit v: R_v^3 <= T, rows by position; else hashed
};

struct HashSizes {
    int64_t S;        // B * H * W * L slots
    int B, H, W, L;
    int NL;           // levels
    int T;            // rows per level, a power of two
};

// one slot's sample at one level: the rows of tap p + 2 q + 4 r and the fractions (nearest: row[0] alone)
template <int FILTER>
struct HashTap {
    int row[FILTER == TEX_LINEAR ? 8 : 1];
    float fx, fy, fz;
};

__device__ __forceinline__ int hg_row(int i, int j, int k, int R, bool dense, uint32_t mask) {
    if (dense) return (k * R + j) * R + i;
    return (int)(((uint32_t)i ^ ((uint32_t)j * 2654435761u) ^ ((uint32_t)k * 805459861u)) & mask);
}

// false = empty slot; (px, py, pz): its position
__device__ __forceinline__ bool hg_live(const HashSizes& z, const HashLevels& lv, int64_t s, const int32_t* __restrict__ layers,
                                        const float* __restrict__ xyz, float& px, float& py, float& pz) {
    if (layers && layers[s] < 0) return false;
    px = xyz[3 * s]; py = xyz[3 * s + 1]; pz = xyz[3 * s + 2];
    const float fn = (float)lv.R[z.NL - 1];
    const float x = px * fn - 0.5f, y = py * fn - 0.5f, w = pz * fn - 0.5f;
    return fabsf(x) < TEX_RANGE && fabsf(y) < TEX_RANGE && fabsf(w) < TEX_RANGE;   // NaN and infinities fail
}

template <int FILTER, int BOUNDARY>
__device__ __forceinline__ void hg_level(int R, bool dense, uint32_t mask, float px, float py, float pz, HashTap<FILTER>& tap) {
    const float fn = (float)R;
    const float x = px * fn - 0.5f, y = py * fn - 0.5f, w = pz * fn - 0.5f;
    if (FILTER == TEX_NEAREST) {
        const int i = tex_addr<BOUNDARY>((int)floorf(x + 0.5f), R), j = tex_addr<BOUNDARY>((int)floorf(y + 0.5f), R);
        const int k = tex_addr<BOUNDARY>((int)floorf(w + 0.5f), R);
        tap.row[0] = hg_row(i, j, k, R, dense, mask);
        tap.fx = tap.fy = tap.fz = 0.0f;
        return;
    }
    const float x0 = floorf(x), y0 = floorf(y), w0 = floorf(w);
    tap.fx = x - x0; tap.fy = y - y0; tap.fz = w - w0;
    const int i0 = (int)x0, j0 = (int)y0, k0 = (int)w0;
    const int ia[2] = {tex_addr<BOUNDARY>(i0, R), tex_addr<BOUNDARY>(i0 + 1, R)};
    const int ja[2] = {tex_addr<BOUNDARY>(j0, R), tex_addr<BOUNDARY>(j0 + 1, R)};
    const int ka[2] = {tex_addr<BOUNDARY>(k0, R), tex_addr<BOUNDARY>(k0 + 1, R)};
#pragma unroll
    for (int t = 0; t < (FILTER == TEX_LINEAR ? 8 : 1); t++) tap.row[t] = hg_row(ia[t & 1], ja[(t >> 1) & 1], ka[(t >> 2) & 1], R, dense, mask);
}

// a row's F features (VEC: the row is aligned to min(16, 4 F) bytes)
template <int F, bool VEC>
__device__ __forceinline__ void hg_load(const float* __restrict__ p, float (&t)[F]) {
    if constexpr (VEC && F == 2) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        t[0] = v.x; t[1] = v.y;
    } else if constexpr (VEC && F >= 4) {
#pragma unroll
        for (int c = 0; c < F; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + c);
            t[c] = v.x; t[c + 1] = v.y; t[c + 2] = v.z; t[c + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < F; c++) t[c] = p[c];
    }
}

template <int F, bool VEC>
__device__ __forceinline__ void hg_store(float* __restrict__ p, const float (&t)[F]) {
    if constexpr (VEC && F == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(t[0], t[1]);
    } else if constexpr (VEC && F >= 4) {
#pragma unroll
        for (int c = 0; c < F; c += 4) *reinterpret_cast<float4*>(p + c) = make_float4(t[c], t[c + 1], t[c + 2], t[c + 3]);
    } else {
#pragma unroll
        for (int c = 0; c < F; c++) p[c] = t[c];
    }
}

template <int FILTER, int BOUNDARY, int F, bool VEC>
__global__ void __launch_bounds__(TEX_BLOCK)
k_hash_grid(HashSizes z, HashLevels lv, const int32_t* __restrict__ layers, const float* __restrict__ xyz,
            const float* __restrict__ table, float* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (s >= z.S) return;
    const int v = blockIdx.y;
    float o[F];
#pragma unroll
    for (int f = 0; f < F; f++) o[f] = 0.0f;
    float px, py, pz;
    if (hg_live(z, lv, s, layers, xyz, px, py, pz)) {
        HashTap<FILTER> tap;
        hg_level<FILTER, BOUNDARY>(lv.R[v], (lv.dense >> v) & 1u, (uint32_t)z.T - 1u, px, py, pz, tap);
        const float* tb = table + (int64_t)v * z.T * F;
        if constexpr (FILTER == TEX_NEAREST) {
            hg_load<F, VEC>(tb + (int64_t)tap.row[0] * F, o);
        } else {
            float t[8][F];
#pragma unroll
            for (int k = 0; k < 8; k++) hg_load<F, VEC>(tb + (int64_t)tap.row[k] * F, t[k]);
#pragma unroll
            for (int f = 0; f < F; f++) {
                const float a0 = tex_bilinear(t[0][f], t[1][f], t[2][f], t[3][f], tap.fx, tap.fy);
                const float a1 = tex_bilinear(t[4][f], t[5][f], t[6][f], t[7][f], tap.fx, tap.fy);
                o[f] = a0 + tap.fz * (a1 - a0);
            }
        }
    }
    hg_store<F, VEC>(out + (s * z.NL + v) * F, o);
}

// (linear only: the entry point zero-fills dL_dxyz for nearest.)  The sums run over a level's features in order; F = 8 takes
// them four at a time, into the same sums.
template <int BOUNDARY, int F, bool VEC>
__global__ void __launch_bounds__(TEX_BLOCK)
k_hash_grid_bwd_xyz(HashSizes z, HashLevels lv, const int32_t* __restrict__ layers, const float* __restrict__ xyz,
                    const float* __restrict__ table, const float* __restrict__ g, float* __restrict__ dL_dxyz) {
    constexpr int FC = F < 4 ? F : 4;
    const int64_t s = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (s >= z.S) return;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    float px, py, pz;
    if (hg_live(z, lv, s, layers, xyz, px, py, pz)) {
        const uint32_t mask = (uint32_t)z.T - 1u;
        const float* gs = g + s * z.NL * F;
#pragma unroll 1
        for (int v = 0; v < z.NL; v++) {
            HashTap<TEX_LINEAR> tap;
            hg_level<TEX_LINEAR, BOUNDARY>(lv.R[v], (lv.dense >> v) & 1u, mask, px, py, pz, tap);
            const float* tb = table + (int64_t)v * z.T * F;
            float su0 = 0.0f, sv0 = 0.0f, su1 = 0.0f, sv1 = 0.0f, sw = 0.0f;
#pragma unroll
            for (int c0 = 0; c0 < F; c0 += FC) {
                float t[8][FC], gv[FC];
#pragma unroll
                for (int k = 0; k < 8; k++) hg_load<FC, VEC>(tb + (int64_t)tap.row[k] * F + c0, t[k]);
                hg_load<FC, VEC>(gs + v * F + c0, gv);
#pragma unroll
                for (int f = 0; f < FC; f++) {
                    tex_uv_term(t[0][f], t[1][f], t[2][f], t[3][f], gv[f], tap.fx, tap.fy, su0, sv0);
                    tex_uv_term(t[4][f], t[5][f], t[6][f], t[7][f], gv[f], tap.fx, tap.fy, su1, sv1);
                    sw += gv[f] * (tex_bilinear(t[4][f], t[5][f], t[6][f], t[7][f], tap.fx, tap.fy) -
                                   tex_bilinear(t[0][f], t[1][f], t[2][f], t[3][f], tap.fx, tap.fy));
                }
            }
            const float fn = (float)lv.R[v];
            gx += fn * (su0 + tap.fz * (su1 - su0));
            gy += fn * (sv0 + tap.fz * (sv1 - sv0));
            gz += fn * sw;
        }
    }
    dL_dxyz[3 * s] = gx; dL_dxyz[3 * s + 1] = gy; dL_dxyz[3 * s + 2] = gz;
}

// blockIdx.z = level * B + view
template <int FILTER, int BOUNDARY, int CH>
__global__ void __launch_bounds__(TILE_PIX)
k_hash_grid_bwd_table(HashSizes z, HashLevels lv, int F, const int32_t* __restrict__ layers, const float* __restrict__ xyz,
                      const float* __restrict__ g, float* __restrict__ dL_dtable) {
    constexpr int NTAP = FILTER == TEX_LINEAR ? 8 : 1;
    __shared__ TexTable<CH> tab;
    const int tid = threadIdx.x;
    const int v = blockIdx.z / z.B, b = blockIdx.z - v * z.B;
    const uint32_t px = blockIdx.x * TILE + (tid & 15), py = blockIdx.y * TILE + (tid >> 4);
    const bool inside = px < (uint32_t)z.W && py < (uint32_t)z.H;
    const int64_t pix = ((int64_t)b * z.H + py) * z.W + px;
    const int L = z.L, R = lv.R[v];
    const bool dense = (lv.dense >> v) & 1u;
    const uint32_t mask = (uint32_t)z.T - 1u;
    float* dst = dL_dtable + (int64_t)v * z.T * F;
    for (int l = 0; l < L; l++) {
        const int64_t s = pix * L + l;
        HashTap<FILTER> tap;
#pragma unroll
        for (int k = 0; k < NTAP; k++) tap.row[k] = 0;
        tap.fx = tap.fy = tap.fz = 0.0f;
        float qx, qy, qz;
        const bool live = inside && hg_live(z, lv, s, layers, xyz, qx, qy, qz);
        if (live) hg_level<FILTER, BOUNDARY>(R, dense, mask, qx, qy, qz, tap);
        // tap p + 2 q + 4 r: weight (wx_p * wy_q) * wz_r
        float w[NTAP];
        if (FILTER == TEX_LINEAR) {
            const float wx[2] = {1.0f - tap.fx, tap.fx}, wy[2] = {1.0f - tap.fy, tap.fy}, wz[2] = {1.0f - tap.fz, tap.fz};
#pragma unroll
            for (int k = 0; k < NTAP; k++) w[k] = (wx[k & 1] * wy[(k >> 1) & 1]) * wz[(k >> 2) & 1];
        } else {
            w[0] = 1.0f;
        }
        // the slot's F upstream values of this level as a row of their own: slot 0 of a (1, F) tensor
        const float* gl = g + (live ? (s * z.NL + v) * F : 0);
        tex_scatter_layer_masked<CH, NTAP, false>(tab, tid, live, tap.row, w, (1u << NTAP) - 1u, 0u, gl, 0, F,
                                                  [&](int k) { return dst + (int64_t)k * F; });
    }
}

static HashSizes hg_sizes(int B, int H, int W, int L, int NL, int T) {
    HashSizes z;
    z.S = (int64_t)B * H * W * L;
    z.B = B; z.H = H; z.W = W; z.L = L; z.NL = NL; z.T = T;
    return z;
}

static HashLevels hg_levels(const int* R, int NL, int T) {
    HashLevels lv;
    lv.dense = 0;
    for (int v = 0; v < HG_MAX_LEVELS; v++) {
        lv.R[v] = v < NL ? R[v] : 1;
        if (v < NL && (int64_t)R[v] * R[v] * R[v] <= (int64_t)T) lv.dense |= 1u << v;
    }
    return lv;
}

#define DM2_HG_F(F, X, ...)                             \
    do {                                                \
        if ((F) == 1) { X(__VA_ARGS__, 1); }            \
        else if ((F) == 2) { X(__VA_ARGS__, 2); }       \
        else if ((F) == 4) { X(__VA_ARGS__, 4); }       \
        else { X(__VA_ARGS__, 8); }                     \
    } while (0)

void launch_hash_grid(int B, int H, int W, int L, int NL, int T, int F, const int* R, int filter, int boundary,
                      const int32_t* render_layers, const float* xyz, const float* table, float* out, hipStream_t st) {
    const HashSizes z = hg_sizes(B, H, W, L, NL, T);
    const HashLevels lv = hg_levels(R, NL, T);
    const dim3 blocks = tex_flat_grid(z.S, (unsigned)NL);
    const uintptr_t align = F >= 4 ? 15 : 4 * F - 1;
    const bool vec = F > 1 && (((uintptr_t)table | (uintptr_t)out) & align) == 0;
#define DM2_HG_FWD(Fl, Bd, Fe)                                                                                                         \
    do {                                                                                                                               \
        if (vec) hipLaunchKernelGGL((k_hash_grid<Fl, Bd, Fe, true>), blocks, dim3(TEX_BLOCK), 0, st, z, lv, render_layers, xyz, table, out);  \
        else hipLaunchKernelGGL((k_hash_grid<Fl, Bd, Fe, false>), blocks, dim3(TEX_BLOCK), 0, st, z, lv, render_layers, xyz, table, out);     \
    } while (0)
#define DM2_HG_FWD_MODES(Fl, Bd) DM2_HG_F(F, DM2_HG_FWD, Fl, Bd)
    DM2_TEX_MODES(filter, boundary, DM2_HG_FWD_MODES);
#undef DM2_HG_FWD_MODES
#undef DM2_HG_FWD
}

void launch_hash_grid_backward(int B, int H, int W, int L, int NL, int T, int F, const int* R, int filter, int boundary,
                               const int32_t* render_layers, const float* xyz, const float* table, const float* dL_dout,
                               float* dL_dtable, float* dL_dxyz, hipStream_t st) {
    const HashSizes z = hg_sizes(B, H, W, L, NL, T);
    const HashLevels lv = hg_levels(R, NL, T);
    if (dL_dxyz) {
        const dim3 blocks = tex_flat_grid(z.S);                             // (linear: the entry point zero-fills for nearest)
        const uintptr_t align = F >= 4 ? 15 : 4 * F - 1;
        const bool vec = F > 1 && (((uintptr_t)table | (uintptr_t)dL_dout) & align) == 0;
#define DM2_HG_XYZ(Bd, Fe)                                                                                                                        \
    do {                                                                                                                                          \
        if (vec) hipLaunchKernelGGL((k_hash_grid_bwd_xyz<Bd, Fe, true>), blocks, dim3(TEX_BLOCK), 0, st, z, lv, render_layers, xyz, table, dL_dout, dL_dxyz);  \
        else hipLaunchKernelGGL((k_hash_grid_bwd_xyz<Bd, Fe, false>), blocks, dim3(TEX_BLOCK), 0, st, z, lv, render_layers, xyz, table, dL_dout, dL_dxyz);     \
    } while (0)
        if (boundary == TEX_WRAP) DM2_HG_F(F, DM2_HG_XYZ, TEX_WRAP);
        else DM2_HG_F(F, DM2_HG_XYZ, TEX_CLAMP);
#undef DM2_HG_XYZ
    }
    if (dL_dtable) {
        const dim3 tiles = tile_grid(W, H, 1);
        const dim3 blocks(tiles.x, tiles.y, (unsigned)(NL * B));
#define DM2_HG_TABLE(Fl, Bd, CH) hipLaunchKernelGGL((k_hash_grid_bwd_table<Fl, Bd, CH>), blocks, dim3(TILE_PIX), 0, st, z, lv, F, render_layers, xyz, dL_dout, dL_dtable)
#define DM2_HG_TABLE_MODES(Fl, Bd)                                      \
    do {                                                                \
        if (F == 1) DM2_HG_TABLE(Fl, Bd, 1);                            \
        else if (F == 2) DM2_HG_TABLE(Fl, Bd, 2);                       \
        else DM2_HG_TABLE(Fl, Bd, TEX_CH);     /* F = 8: two chunks */  \
    } while (0)
        DM2_TEX_MODES(filter, boundary, DM2_HG_TABLE_MODES);
#undef DM2_HG_TABLE_MODES
#undef DM2_HG_TABLE
    }
}

}  // namespace dm2
