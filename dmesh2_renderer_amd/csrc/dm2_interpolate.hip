// dm2_interpolate.hip -- Renderer.interpolate: attribute images from rasterize's hits (face id + barycentrics per slot):
//   k_interpolate            out[s, c] = (bary[s,0] attr[v0,c] + bary[s,1] attr[v1,c]) + bary[s,2] attr[v2,c]
//   k_interpolate_bwd_bary   dL/dbary[s, k] = sum_c attr[v_k, c] g[s, c]
//   k_interpolate_bwd_attr   dL/dattr[v_k, c] += bary[s, k] g[s, c]
//
// Contract (include/dm2_hip.h, dm2_interpolate): a slot s = (b, y, x, l) is filled when f = render_layers[s] lies in [0, F)
// and the three rows v_k = attr_faces[f][k] lie in [0, N); every other slot is empty: zeros out, nothing read through its
// bary, no gradient.  -ffp-contract=off: the forward is a pure function of the written operation order.
//
// Forward and bary backward: the slots are a flat list (the tile shape does not matter to a gather).  A block takes 256
// consecutive slots; each lane reads one slot's id, attr_faces row and bary once and stages them in LDS, then the block
// sweeps its 256 * C outputs (3 * 256 for the bary gradient) with consecutive lanes on consecutive floats: the stores of a
// wave are contiguous, and the lanes of one slot read consecutive channels of the same three attr rows.
//
// attr backward: the scatter.  One block per 16 x 16 pixel tile and view (neighbouring pixels list the same faces), one lane
// per pixel, the channels in chunks of CH.  A (slot, vertex, channel) contribution goes into the face's slot of the block's
// FaceTable (dm2_face_table.h; 3 x CH fp32 accumulators per slot, a padded stride so that neither the lanes of the accumulation
// nor those of the flush meet in a bank), flushed by slot: consecutive lanes on consecutive channels of one attr row.  The keys
// stay from chunk to chunk, so a face keeps its slot.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"

namespace dm2 {

constexpr int IP_BLOCK = 256;             // slots per block of the flat kernels
constexpr int IP_CH = 4;                  // the longest channel chunk of the attr backward
constexpr int IP_STRIDE = LC_SLOTS + 1;   // accumulator stride per component: bank = (component + slot) % 64

struct InterpSizes {
    int64_t S;        // B * H * W * L slots
    int64_t per_view; // slots per view (H * W * L)
    int B, H, W, L, F, N, C;
    int view_tables;  // attr is (B, N, C): row v of view b is row b * N + v
};

// the three attr rows of slot s (view offset included), false = empty slot
__device__ __forceinline__ bool ip_rows(const InterpSizes& z, int64_t s, const int32_t* __restrict__ layers,
                                        const int32_t* __restrict__ attr_faces, int rows[3]) {
    const int f = layers[s];
    if ((unsigned)f >= (unsigned)z.F) return false;
    const int r0 = attr_faces[3 * (int64_t)f], r1 = attr_faces[3 * (int64_t)f + 1], r2 = attr_faces[3 * (int64_t)f + 2];
    if ((unsigned)r0 >= (unsigned)z.N || (unsigned)r1 >= (unsigned)z.N || (unsigned)r2 >= (unsigned)z.N) return false;
    const int base = z.view_tables ? (int)(s / z.per_view) * z.N : 0;          // B * N < 2^31: checked by the entry point
    rows[0] = base + r0; rows[1] = base + r1; rows[2] = base + r2;
    return true;
}

__global__ void __launch_bounds__(IP_BLOCK)
k_interpolate(InterpSizes z, const int32_t* __restrict__ layers, const float* __restrict__ bary, const float* __restrict__ attr,
              const int32_t* __restrict__ attr_faces, float* __restrict__ out) {
    __shared__ int s_row[3][IP_BLOCK];
    __shared__ float s_w[3][IP_BLOCK];
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * IP_BLOCK;
    const int nslots = (int)min((int64_t)IP_BLOCK, z.S - s0);
    if (tid < nslots) {
        const int64_t s = s0 + tid;
        int rows[3] = {-1, -1, -1};
        float w[3] = {0.0f, 0.0f, 0.0f};
        if (ip_rows(z, s, layers, attr_faces, rows)) { w[0] = bary[3 * s]; w[1] = bary[3 * s + 1]; w[2] = bary[3 * s + 2]; }
#pragma unroll
        for (int k = 0; k < 3; k++) { s_row[k][tid] = rows[k]; s_w[k][tid] = w[k]; }
    }
    __syncthreads();
    const int C = z.C, total = nslots * C;
    const int dq = IP_BLOCK / C, dr = IP_BLOCK - dq * C;                      // the step of (slot, channel) per sweep
    int slot = tid / C, c = tid - slot * C;
    float* o = out + s0 * C;
    for (int e = tid; e < total; e += IP_BLOCK) {
        const int r0 = s_row[0][slot];
        float v = 0.0f;
        if (r0 >= 0) {
            const float a0 = attr[(int64_t)r0 * C + c], a1 = attr[(int64_t)s_row[1][slot] * C + c], a2 = attr[(int64_t)s_row[2][slot] * C + c];
            v = (s_w[0][slot] * a0 + s_w[1][slot] * a1) + s_w[2][slot] * a2;
        }
        o[e] = v;
        slot += dq; c += dr;
        if (c >= C) { c -= C; slot++; }
    }
}

// VEC4: C is a multiple of 4 and attr / g are 16-byte aligned, so the rows are read four channels at a time; the sum runs over
// the channels in the same order either way (the same bits).
template <bool VEC4>
__global__ void __launch_bounds__(IP_BLOCK)
k_interpolate_bwd_bary(InterpSizes z, const int32_t* __restrict__ layers, const float* __restrict__ attr,
                       const int32_t* __restrict__ attr_faces, const float* __restrict__ g, float* __restrict__ dL_dbary) {
    __shared__ int s_row[3 * IP_BLOCK];                                       // [slot][k]: the order of the outputs
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * IP_BLOCK;
    const int nslots = (int)min((int64_t)IP_BLOCK, z.S - s0);
    if (tid < nslots) {
        int rows[3] = {-1, -1, -1};
        ip_rows(z, s0 + tid, layers, attr_faces, rows);
#pragma unroll
        for (int k = 0; k < 3; k++) s_row[3 * tid + k] = rows[k];
    }
    __syncthreads();
    const int C = z.C;
    for (int e = tid; e < 3 * nslots; e += IP_BLOCK) {
        const int row = s_row[e];
        float acc = 0.0f;
        if (row >= 0) {
            const float* a = attr + (int64_t)row * C;
            const float* gs = g + (s0 + e / 3) * C;
            if (VEC4) {
                const float4* a4 = reinterpret_cast<const float4*>(a);
                const float4* g4 = reinterpret_cast<const float4*>(gs);
                for (int c = 0; c < C / 4; c++) {
                    const float4 x = a4[c], y = g4[c];
                    acc += x.x * y.x; acc += x.y * y.y; acc += x.z * y.z; acc += x.w * y.w;
                }
            } else {
                for (int c = 0; c < C; c++) acc += a[c] * gs[c];
            }
        }
        dL_dbary[3 * s0 + e] = acc;
    }
}

template <int CH>
__global__ void __launch_bounds__(TILE_PIX)
k_interpolate_bwd_attr(InterpSizes z, const int32_t* __restrict__ layers, const float* __restrict__ bary,
                       const int32_t* __restrict__ attr_faces, const float* __restrict__ g, float* __restrict__ dL_dattr) {
    __shared__ FaceTable<float, 3 * CH, IP_STRIDE> tab;                       // component k * CH + c
    const int b = blockIdx.z, tid = threadIdx.x;
    tab.clear_keys(tid);
    const TilePixel t = tile_pixel(tid, z.W, z.H);
    const int C = z.C, L = z.L;
    float* dst = dL_dattr + (z.view_tables ? (int64_t)b * z.N * C : 0);
    for (int c0 = 0; c0 < C; c0 += CH) {
        const int nc = min(CH, C - c0);
        tab.clear_acc(tid);
        __syncthreads();
        if (t.inside) {
            for (int l = 0; l < L; l++) {
                const int64_t s = t.pix * L + l;
                const int f = layers[s];
                if ((unsigned)f >= (unsigned)z.F) continue;
                const int r[3] = {attr_faces[3 * (int64_t)f], attr_faces[3 * (int64_t)f + 1], attr_faces[3 * (int64_t)f + 2]};
                if ((unsigned)r[0] >= (unsigned)z.N || (unsigned)r[1] >= (unsigned)z.N || (unsigned)r[2] >= (unsigned)z.N) continue;
                const float w[3] = {bary[3 * s], bary[3 * s + 1], bary[3 * s + 2]};
                float gv[CH];
#pragma unroll
                for (int c = 0; c < CH; c++) gv[c] = c < nc ? g[s * C + c0 + c] : 0.0f;
                const int slot = tab.slot(f);
#pragma unroll
                for (int k = 0; k < 3; k++) {
#pragma unroll
                    for (int c = 0; c < CH; c++) {
                        if (c >= nc) continue;
                        const float v = w[k] * gv[c];
                        if (slot >= 0) tab.add(slot, k * CH + c, v);
                        else atomicAdd(dst + (int64_t)r[k] * C + c0 + c, v);
                    }
                }
            }
        }
        __syncthreads();
        // flush: one global atomic per (attr row, channel) of every face the tile listed; lane -> (slot, k, c), c fastest
        tab.flush_by_slot(tid, [&](int f, int comp, float v) {
            const int k = comp / CH, c = comp - k * CH;
            if (c >= nc) return;
            atomicAdd(dst + (int64_t)attr_faces[3 * (int64_t)f + k] * C + c0 + c, v);
        });
        __syncthreads();
    }
}

static InterpSizes ip_sizes(int B, int H, int W, int L, int F, int N, int C, int view_tables) {
    InterpSizes z;
    z.per_view = (int64_t)H * W * L;
    z.S = (int64_t)B * z.per_view;
    z.B = B; z.H = H; z.W = W; z.L = L; z.F = F; z.N = N; z.C = C; z.view_tables = view_tables;
    return z;
}

void launch_interpolate(int B, int H, int W, int L, int F, int N, int C, int view_tables, const int32_t* render_layers,
                        const float* bary, const float* attr, const int32_t* attr_faces, float* out, hipStream_t st) {
    const InterpSizes z = ip_sizes(B, H, W, L, F, N, C, view_tables);
    const dim3 grid((unsigned)((z.S + IP_BLOCK - 1) / IP_BLOCK));
    hipLaunchKernelGGL(k_interpolate, grid, dim3(IP_BLOCK), 0, st, z, render_layers, bary, attr, attr_faces, out);
}

void launch_interpolate_backward(int B, int H, int W, int L, int F, int N, int C, int view_tables, const int32_t* render_layers,
                                 const float* bary, const float* attr, const int32_t* attr_faces, const float* dL_dout,
                                 float* dL_dattr, float* dL_dbary, hipStream_t st) {
    const InterpSizes z = ip_sizes(B, H, W, L, F, N, C, view_tables);
    if (dL_dbary) {
        const dim3 grid((unsigned)((z.S + IP_BLOCK - 1) / IP_BLOCK));
        const bool vec4 = C % 4 == 0 && (((uintptr_t)attr | (uintptr_t)dL_dout) & 15) == 0;
        if (vec4) hipLaunchKernelGGL(k_interpolate_bwd_bary<true>, grid, dim3(IP_BLOCK), 0, st, z, render_layers, attr, attr_faces, dL_dout, dL_dbary);
        else hipLaunchKernelGGL(k_interpolate_bwd_bary<false>, grid, dim3(IP_BLOCK), 0, st, z, render_layers, attr, attr_faces, dL_dout, dL_dbary);
    }
    if (dL_dattr) {
        const dim3 grid = tile_grid(W, H, B);
#define DM2_IP_LAUNCH(CH) \
    hipLaunchKernelGGL(k_interpolate_bwd_attr<CH>, grid, dim3(TILE_PIX), 0, st, z, render_layers, bary, attr_faces, dL_dout, dL_dattr)
        if (C == 1) DM2_IP_LAUNCH(1);
        else if (C == 2) DM2_IP_LAUNCH(2);
        else if (C == 3) DM2_IP_LAUNCH(3);
        else DM2_IP_LAUNCH(IP_CH);
#undef DM2_IP_LAUNCH
    }
}

}  // namespace dm2
