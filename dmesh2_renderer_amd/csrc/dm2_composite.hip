// dm2_composite.hip -- Renderer.composite: per-slot values (B,H,W,L,C) blended front to back into an image (B,H,W,C):
//   k_composite       O_c = O_c + values[l,c] * (a_l * T),  T = T * (1 - a_l),  stop at T < T_EPS;  out = O + T * background
//   k_composite_bwd   dL/dvalues[l,c] = (a_l T_l) g_c;  dL/da_l = T_l (S_l - R),  R <- a_l S_l + (1 - a_l) R  from R = K backwards,
//                     S_l = sum_c g_c values[l,c],  K = sum_c g_c background_c - gA
//
// Contract (include/dm2_hip.h, dm2_composite): a slot is empty when its id is negative (per-face alpha: outside [0, F));
// neither the values nor the alpha of an empty slot, nor anything behind the stop, takes part (a mask of the blended slots,
// not "w == 0", decides what is read: a blended slot with a == 0 still adds values * 0).  -ffp-contract=off: the forward is a
// pure function of the written operation order.
//
// A pixel's data is L * C contiguous floats, so one lane per pixel walking (l, c) would read with a stride of L * C floats
// between lanes.  Both kernels therefore split the work as dm2_interpolate.hip does: a scalar phase with one lane per pixel
// (ids, alphas, the recurrence) parks per-slot weights in LDS ([pixel][slot] with an odd stride: the lanes of the scalar
// phase meet in no bank), then the block sweeps its pixels x C (x L) floats with consecutive lanes on consecutive floats
// (four floats per lane on the vector path).  L is arbitrary: the slots go in chunks of CP_LCH, the lane keeps T between the
// chunks, and from the second chunk on the sweep takes up the partial sum it stored itself (L <= CP_LCH: one pass, no
// read-back).  The backward walks the chunks from the last to the first (the back pass starts at the last blended slot) and
// recomputes T from the front for every chunk.
//
// Forward: a block takes 256 consecutive pixels.  Backward, per-slot alpha: the same.  Backward, per-face alpha: one block per
// 16 x 16 pixel tile and view (neighbouring pixels list the same faces); dL/da_l goes into the face's slot of the block's
// FaceTable (dm2_face_table.h; one fp32 accumulator per slot) and the block flushes with one global atomic per face of the
// tile; a face that finds no slot adds straight to global memory.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"

namespace dm2 {

constexpr int CP_PIX = 256;               // pixels per block (TILE_PIX of the tiled backward)
constexpr int CP_LCH = 8;                 // slots per chunk (a multiple of 4: the vector loads of the ids)
constexpr int CP_SL = CP_LCH + 1;         // LDS stride per pixel: odd, bank = (9 pixel + slot) % 64
static_assert(CP_PIX == TILE_PIX && CP_LCH % 4 == 0, "the tiled backward is one lane per pixel of a 16 x 16 tile");

struct CompSizes {
    int64_t P;        // B * H * W pixels
    int B, H, W, L, C, F;
};

// global index of the block's pixel p (0 .. 255), -1 beyond the image
template <bool TILED>
__device__ __forceinline__ int64_t cp_pixel(const CompSizes& z, int p) {
    if (TILED) {
        const uint32_t px = blockIdx.x * TILE + (p & 15), py = blockIdx.y * TILE + (p >> 4);
        if (px >= (uint32_t)z.W || py >= (uint32_t)z.H) return -1;
        return ((int64_t)blockIdx.z * z.H + py) * z.W + px;
    }
    const int64_t g = (int64_t)blockIdx.x * CP_PIX + p;
    return g < z.P ? g : -1;
}

// slots s .. s + LVEC - 1 (LVEC = 4: L is a multiple of 4 and the arrays are 16-byte aligned): live = not empty, a = its alpha
template <bool FACE, int LVEC>
__device__ __forceinline__ void cp_load(const CompSizes& z, int64_t s, const int32_t* __restrict__ layers,
                                        const float* __restrict__ alpha, int id[LVEC], bool live[LVEC], float a[LVEC]) {
    if (!layers) {
#pragma unroll
        for (int k = 0; k < LVEC; k++) id[k] = 0;
    } else if (LVEC == 4) {
        const int4 q = *reinterpret_cast<const int4*>(layers + s);
        id[0] = q.x; id[1 % LVEC] = q.y; id[2 % LVEC] = q.z; id[3 % LVEC] = q.w;
    } else {
        id[0] = layers[s];
    }
    if (FACE) {
#pragma unroll
        for (int k = 0; k < LVEC; k++) {
            live[k] = (unsigned)id[k] < (unsigned)z.F;
            a[k] = live[k] ? alpha[id[k]] : 0.0f;
        }
    } else if (LVEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(alpha + s);
        a[0] = q.x; a[1 % LVEC] = q.y; a[2 % LVEC] = q.z; a[3 % LVEC] = q.w;
#pragma unroll
        for (int k = 0; k < LVEC; k++) live[k] = id[k] >= 0;
    } else {
        live[0] = id[0] >= 0;
        a[0] = live[0] ? alpha[s] : 0.0f;
    }
}

// VEC4: C is a multiple of 4 and values / out are 16-byte aligned, so a lane takes four channels at a time; every channel goes
// through the same operations either way (the same bits).
template <bool FACE, int LVEC, bool VEC4>
__global__ void __launch_bounds__(CP_PIX)
k_composite(CompSizes z, const float* __restrict__ values, const float* __restrict__ alpha, const int32_t* __restrict__ layers,
            const float* __restrict__ background, float* __restrict__ out, float* __restrict__ out_acc,
            float* __restrict__ out_final_T, int32_t* __restrict__ out_n_contrib) {
    __shared__ float s_w[CP_PIX * CP_SL];
    __shared__ uint32_t s_mask[CP_PIX];                                       // bit l: slot l0 + l blended
    __shared__ float s_T[CP_PIX];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * CP_PIX;
    const int npix = (int)min((int64_t)CP_PIX, z.P - p0);
    const int L = z.L, C = z.C;
    constexpr int V = VEC4 ? 4 : 1;
    const int CV = C / V, total = npix * CV;                                  // lane -> (pixel, group of V channels), group fastest
    float T = 1.0f;
    int n = 0;
    bool done = false;
    int l0 = 0;
    do {
        const int lc = min(CP_LCH, L - l0);
        const bool last = l0 + lc >= L;
        if (tid < npix) {
            uint32_t mask = 0;
            const int64_t s0 = (p0 + tid) * L + l0;
            for (int l = 0; l < lc && !done; l += LVEC) {
                int id[LVEC];
                bool live[LVEC];
                float a[LVEC];
                cp_load<FACE, LVEC>(z, s0 + l, layers, alpha, id, live, a);
#pragma unroll
                for (int k = 0; k < LVEC; k++) {
                    if (!live[k] || done) continue;
                    s_w[tid * CP_SL + l + k] = a[k] * T;
                    mask |= 1u << (l + k);
                    T = T * (1.0f - a[k]);
                    n = l0 + l + k + 1;
                    if (T < T_EPS) done = true;
                }
            }
            s_mask[tid] = mask;
            if (last) {
                s_T[tid] = T;
                if (out_final_T) out_final_T[p0 + tid] = T;
                if (out_n_contrib) out_n_contrib[p0 + tid] = n;
                if (out_acc) out_acc[p0 + tid] = 1.0f - T;
            }
        }
        __syncthreads();
        for (int e = tid; e < total; e += CP_PIX) {
            const int p = e / CV, c = (e - p * CV) * V;
            float* dst = out + (p0 + p) * C + c;
            float o[V];
            if (l0 == 0) {
#pragma unroll
                for (int k = 0; k < V; k++) o[k] = 0.0f;
            } else if (VEC4) {                                                // the partial sum this lane stored for the chunks before
                const float4 q = *reinterpret_cast<const float4*>(dst);
                o[0] = q.x; o[1 % V] = q.y; o[2 % V] = q.z; o[3 % V] = q.w;
            } else {
                o[0] = *dst;
            }
            const uint32_t mask = s_mask[p];
            const float* v = values + ((p0 + p) * L + l0) * C + c;
            for (int l = 0; (mask >> l) != 0; l++) {
                if (!((mask >> l) & 1u)) continue;
                const float w = s_w[p * CP_SL + l];
                if (VEC4) {
                    const float4 x = *reinterpret_cast<const float4*>(v + (int64_t)l * C);
                    o[0] = o[0] + x.x * w; o[1 % V] = o[1 % V] + x.y * w; o[2 % V] = o[2 % V] + x.z * w; o[3 % V] = o[3 % V] + x.w * w;
                } else {
                    o[0] = o[0] + v[(int64_t)l * C] * w;
                }
            }
            if (last && background) {
                const float Tp = s_T[p];
#pragma unroll
                for (int k = 0; k < V; k++) o[k] = o[k] + Tp * background[c + k];
            }
            if (VEC4) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1 % V], o[2 % V], o[3 % V]);
            else *dst = o[0];
        }
        l0 += CP_LCH;
        if (l0 < L) __syncthreads();
    } while (l0 < L);
}

// FACE: per-face alpha, 16 x 16 tiles, dL/dalpha (F) through the face table; otherwise 256 consecutive pixels and a dense
// dL/dalpha (B,H,W,L).  g, gA, dL_dvalues and dL_dalpha may each be NULL (a missing upstream is zero; a gradient nobody asked
// for runs no phase of its own).  VEC4 as in k_composite (values, g and dL_dvalues aligned): the sums run over the channels in
// the same order either way.
template <bool FACE, bool VEC4>
__global__ void __launch_bounds__(CP_PIX)
k_composite_bwd(CompSizes z, const float* __restrict__ values, const float* __restrict__ alpha, const int32_t* __restrict__ layers,
                const float* __restrict__ background, const int32_t* __restrict__ n_contrib, const float* __restrict__ g,
                const float* __restrict__ gA, float* __restrict__ dL_dvalues, float* __restrict__ dL_dalpha) {
    __shared__ float s_a[CP_PIX * CP_SL], s_Tl[CP_PIX * CP_SL];              // alpha and the transmittance in front of a blended slot
    __shared__ float s_S[CP_PIX * CP_SL];                                     // S_l, then dL/da_l
    __shared__ uint32_t s_mask[CP_PIX];
    FaceTable<float, 1>* tab = nullptr;                                        // FACE only: otherwise none is declared
    if constexpr (FACE) { __shared__ FaceTable<float, 1> s_tab; tab = &s_tab; }
    const int tid = threadIdx.x;
    const int L = z.L, C = z.C;
    constexpr int V = VEC4 ? 4 : 1;
    const int CV = C / V;
    const int64_t gp = cp_pixel<FACE>(z, tid);
    if constexpr (FACE) tab->clear(tid);
    const int n = gp >= 0 ? n_contrib[gp] : 0;                                 // blended: not empty and in front of slot n
    float R = 0.0f;                                                            // the back pass's carry, K at its start
    if (dL_dalpha && n > 0) {
        if (g && background)
            for (int c = 0; c < C; c++) R += g[gp * C + c] * background[c];
        if (gA) R = R - gA[gp];
    }
    for (int l0 = ((L - 1) / CP_LCH) * CP_LCH; l0 >= 0; l0 -= CP_LCH) {
        const int lc = min(CP_LCH, L - l0);
        // B1, one lane per pixel: T front to back up to the end of this chunk
        uint32_t mask = 0;
        if (n > l0) {
            float T = 1.0f;
            const int end = min(n, l0 + lc);
            for (int l = 0; l < end; l++) {
                int id[1];
                bool live[1];
                float a[1];
                cp_load<FACE, 1>(z, gp * L + l, layers, alpha, id, live, a);
                if (!live[0]) continue;
                if (l >= l0) {
                    s_a[tid * CP_SL + l - l0] = a[0];
                    s_Tl[tid * CP_SL + l - l0] = T;
                    mask |= 1u << (l - l0);
                }
                T = T * (1.0f - a[0]);
            }
        }
        s_mask[tid] = mask;
        __syncthreads();
        if (dL_dalpha) {
            // A: S_l of every blended slot, lane -> (pixel, slot), a sequential sum over the channels
            for (int e = tid; e < CP_PIX * lc; e += CP_PIX) {
                const int p = e / lc, l = e - p * lc;
                if (!((s_mask[p] >> l) & 1u)) continue;
                float S = 0.0f;
                if (g) {
                    const int64_t q = cp_pixel<FACE>(z, p);
                    const float* v = values + (q * L + l0 + l) * C;
                    const float* gs = g + q * C;
                    if (VEC4) {
                        for (int c = 0; c < C; c += 4) {
                            const float4 x = *reinterpret_cast<const float4*>(v + c), y = *reinterpret_cast<const float4*>(gs + c);
                            S += y.x * x.x; S += y.y * x.y; S += y.z * x.z; S += y.w * x.w;
                        }
                    } else {
                        for (int c = 0; c < C; c++) S += gs[c] * v[c];
                    }
                }
                s_S[p * CP_SL + l] = S;
            }
            __syncthreads();
            // B2, one lane per pixel: the back pass over this chunk
            for (int l = lc - 1; l >= 0; l--) {
                float d = 0.0f;
                if ((mask >> l) & 1u) {
                    const float a = s_a[tid * CP_SL + l], S = s_S[tid * CP_SL + l];
                    d = s_Tl[tid * CP_SL + l] * (S - R);
                    R = a * S + (1.0f - a) * R;
                    if constexpr (FACE) {
                        const int f = layers[gp * L + l0 + l];
                        const int slot = tab->slot(f);
                        if (slot >= 0) tab->add(slot, 0, d);
                        else atomicAdd(dL_dalpha + f, d);
                    }
                }
                if (!FACE) s_S[tid * CP_SL + l] = d;
            }
            if (!FACE) {
                __syncthreads();
                for (int e = tid; e < CP_PIX * lc; e += CP_PIX) {             // the dense store: runs of lc floats per pixel
                    const int p = e / lc, l = e - p * lc;
                    const int64_t q = cp_pixel<FACE>(z, p);
                    if (q >= 0) dL_dalpha[q * L + l0 + l] = s_S[p * CP_SL + l];
                }
            }
        }
        if (dL_dvalues) {
            // C: w_l g_c, zeros included; lane -> (pixel, slot, group of V channels), group fastest
            const int X = lc * CV;
            for (int e = tid; e < CP_PIX * X; e += CP_PIX) {
                const int p = e / X, j = e - p * X;
                const int l = j / CV, c = (j - l * CV) * V;
                const int64_t q = cp_pixel<FACE>(z, p);
                if (q < 0) continue;
                float r[V];
#pragma unroll
                for (int k = 0; k < V; k++) r[k] = 0.0f;
                if (g && ((s_mask[p] >> l) & 1u)) {
                    const float w = s_a[p * CP_SL + l] * s_Tl[p * CP_SL + l];
                    const float* gs = g + q * C + c;
                    if (VEC4) {
                        const float4 y = *reinterpret_cast<const float4*>(gs);
                        r[0] = w * y.x; r[1 % V] = w * y.y; r[2 % V] = w * y.z; r[3 % V] = w * y.w;
                    } else {
                        r[0] = w * gs[0];
                    }
                }
                float* dst = dL_dvalues + (q * L + l0 + l) * C + c;
                if (VEC4) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1 % V], r[2 % V], r[3 % V]);
                else *dst = r[0];
            }
        }
        __syncthreads();
    }
    // flush: one global atomic per face the tile blended
    if constexpr (FACE) { if (dL_dalpha) tab->flush_by_slot(tid, [&](int f, int, float v) { atomicAdd(dL_dalpha + f, v); }); }
}

static CompSizes cp_sizes(int B, int H, int W, int L, int C, int F) {
    CompSizes z;
    z.P = (int64_t)B * H * W;
    z.B = B; z.H = H; z.W = W; z.L = L; z.C = C; z.F = F;
    return z;
}

static bool cp_aligned16(const void* a, const void* b, const void* c) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0; }

void launch_composite(int B, int H, int W, int L, int C, int F, int per_face, const float* values, const float* alpha,
                      const int32_t* render_layers, const float* background, float* out, float* out_acc, float* out_final_T,
                      int32_t* out_n_contrib, hipStream_t st) {
    const CompSizes z = cp_sizes(B, H, W, L, C, F);
    const dim3 grid((unsigned)((z.P + CP_PIX - 1) / CP_PIX));
    const bool vec4 = C % 4 == 0 && cp_aligned16(values, out, nullptr);
    const bool lvec = L > 0 && L % 4 == 0 && cp_aligned16(render_layers, per_face ? nullptr : alpha, nullptr);
#define DM2_CP_FWD(FACE, LV, V4)                                                                                           \
    hipLaunchKernelGGL((k_composite<FACE, LV, V4>), grid, dim3(CP_PIX), 0, st, z, values, alpha, render_layers, background, \
                       out, out_acc, out_final_T, out_n_contrib)
#define DM2_CP_FWD_V(FACE, LV) do { if (vec4) DM2_CP_FWD(FACE, LV, true); else DM2_CP_FWD(FACE, LV, false); } while (0)
    if (per_face) { if (lvec) DM2_CP_FWD_V(true, 4); else DM2_CP_FWD_V(true, 1); }
    else { if (lvec) DM2_CP_FWD_V(false, 4); else DM2_CP_FWD_V(false, 1); }
#undef DM2_CP_FWD_V
#undef DM2_CP_FWD
}

void launch_composite_backward(int B, int H, int W, int L, int C, int F, int per_face, const float* values, const float* alpha,
                               const int32_t* render_layers, const float* background, const int32_t* n_contrib,
                               const float* dL_dout, const float* dL_dacc, float* dL_dvalues, float* dL_dalpha, hipStream_t st) {
    const CompSizes z = cp_sizes(B, H, W, L, C, F);
    const bool vec4 = C % 4 == 0 && cp_aligned16(values, dL_dout, dL_dvalues);
#define DM2_CP_BWD(FACE, V4)                                                                                                 \
    hipLaunchKernelGGL((k_composite_bwd<FACE, V4>), grid, dim3(CP_PIX), 0, st, z, values, alpha, render_layers, background, \
                       n_contrib, dL_dout, dL_dacc, dL_dvalues, dL_dalpha)
    if (per_face) {
        const dim3 grid = tile_grid(W, H, B);
        if (vec4) DM2_CP_BWD(true, true); else DM2_CP_BWD(true, false);
    } else {
        const dim3 grid((unsigned)((z.P + CP_PIX - 1) / CP_PIX));
        if (vec4) DM2_CP_BWD(false, true); else DM2_CP_BWD(false, false);
    }
#undef DM2_CP_BWD
}

}  // namespace dm2
