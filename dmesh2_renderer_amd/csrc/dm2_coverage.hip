// dm2_coverage.hip -- Renderer.coverage: the analytic triangle-pixel overlap of every listed slot, the factor that turns a
// face's opacity into an anti-aliased alpha on the deferred path (rasterize -> interpolate -> texture -> composite):
//   k_coverage       cov[s] = mix_coverage(code, area(tri(f), pixel), temperature), 0 in an empty slot, where the clipper errs and
//                    where area == 0 (Renderer.forward skips such a face, forward.cu:337); code = 0 (a hit), or -- with the
//                    `inside` mask of rasterize's overlap mode -- 1 where inside[s] == 0: area * temperature, forward's mix of
//                    a face that only grazes the pixel (forward.cu:379-381)
//   k_coverage_bwd   dL/dverts_image[b, v_k] += g_cov[s] * temperature * d(area)/d(corner k), the CCW reorder undone
//
// Contract (include/dm2_hip.h, dm2_coverage).  The triangle is verts_image[b, faces[f]]; its six AA tables are built in
// registers in pack_face's operation order under DM2_FLAG_TABLES_FROM_IMAGE (dm2_stage.h; bit-identical to the fused host
// prep's k_aa_tables), the pixel is [x, x+1] x [y, y+1], and -ffp-contract=off makes the forward a pure function of the written
// operation order.  Whether the pixel's ray hits the face is not looked at: any listed id gets its area.
//
// Both kernels: one block per 16 x 16 pixel tile and view, one lane per pixel, a loop over the L slots.  Neighbouring pixels
// list the same few faces, so the gathers (three faces entries, three float2 of verts_image per slot) hit in cache.  The
// forward clips with the straight-line area-only clipper (dm2_clip_area.h); the backward re-clips with the reference-shaped
// clipper and its Jacobian (tri_pix_overlap_area<true>, bit-equal to the oracle's), adds the six components into the face's
// slot of the block's FaceTable (dm2_face_table.h) -- stored per VERTEX of the face, the reorder already undone -- and the block
// flushes by slot, with one global atomic per (vertex row, component) and face of the tile (consecutive lanes on x and y of
// one vertex); a face that finds no slot adds straight to global memory.
#include <hip/hip_runtime.h>

#include "dm2_clip_area.h"
#include "dm2_cov_tables.h"
#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"

namespace dm2 {

struct CovSizes {
    int B, H, W, L, P, F;
    float temp;
};

// the three vertex ids of slot id f; false: the slot is empty (f outside [0, F), or a vertex id outside [0, P))
__device__ __forceinline__ bool cov_face(const CovSizes& z, int f, const int32_t* __restrict__ faces, int vid[3]) {
    if ((unsigned)f >= (unsigned)z.F) return false;
    vid[0] = faces[3 * (int64_t)f]; vid[1] = faces[3 * (int64_t)f + 1]; vid[2] = faces[3 * (int64_t)f + 2];
    return (unsigned)vid[0] < (unsigned)z.P && (unsigned)vid[1] < (unsigned)z.P && (unsigned)vid[2] < (unsigned)z.P;
}

// Clamp codes (0: the ray hits the face, 1: it does not) of slots s .. s + LVEC - 1 from the `inside` bytes; !MASK: hits.
// LVEC = 4: the four bytes are one aligned word.
template <int LVEC, bool MASK>
__device__ __forceinline__ void cov_codes(const uint8_t* __restrict__ in_mask, int64_t s, int code[LVEC]) {
#pragma unroll
    for (int k = 0; k < LVEC; k++) code[k] = 0;
    if (!MASK) return;
    if (LVEC == 4) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(in_mask + s);
#pragma unroll
        for (int k = 0; k < LVEC; k++) code[k] = ((q >> (8 * k)) & 0xFFu) == 0u ? 1 : 0;
    } else {
        code[0] = in_mask[s] == 0 ? 1 : 0;
    }
}

// ids of slots s .. s + LVEC - 1 (LVEC = 4: L is a multiple of 4 and the array is 16-byte aligned)
template <int LVEC>
__device__ __forceinline__ void cov_ids(const int32_t* __restrict__ layers, int64_t s, int id[LVEC]) {
    if (LVEC == 4) {
        const int4 q = *reinterpret_cast<const int4*>(layers + s);
        id[0] = q.x; id[1 % LVEC] = q.y; id[2 % LVEC] = q.z; id[3 % LVEC] = q.w;
    } else {
        id[0] = layers[s];
    }
}

// LVEC = 4: render_layers and out are 16-byte aligned (in_mask, when given, 4-byte aligned) and L is a multiple of 4; every
// slot goes through the same operations either way (the same bits).  Every slot of every pixel of the image is written.
// MASK: in_mask is given.  A template parameter, not a test of the pointer: the code array costs the kernel 6 to 8 VGPRs and a
// wave per SIMD, which the call without a mask does not pay (!MASK compiles to the registers of the kernel before the mask).
template <int LVEC, bool MASK>
__global__ void __launch_bounds__(TILE_PIX)
k_coverage(CovSizes z, const int32_t* __restrict__ patch_min, const int32_t* __restrict__ layers, const uint8_t* __restrict__ in_mask, const float* __restrict__ image,
           const int32_t* __restrict__ faces, float* __restrict__ out) {
    const auto [px, py, inside, pix] = tile_pixel(threadIdx.x, z.W, z.H);
    if (!inside) return;
    const int b = blockIdx.z;
    const WinOrigin org = window_origin(patch_min);       // (the pixel's square lies in the frame: verts_image's units)
    const int64_t s0 = pix * z.L;
    const float2* im = reinterpret_cast<const float2*>(image) + (int64_t)b * z.P;
    const float pxmin = (float)(px + org.x), pxmax = pxmin + 1, pymin = (float)(py + org.y), pymax = pymin + 1;
    const float pix_area = 1.0f;
    const float temp = z.temp;
    for (int l = 0; l < z.L; l += LVEC) {
        int id[LVEC], code[LVEC];
        float c[LVEC];
        cov_ids<LVEC>(layers, s0 + l, id);
        cov_codes<LVEC, MASK>(in_mask, s0 + l, code);
#pragma unroll
        for (int k = 0; k < LVEC; k++) {
            c[k] = 0.0f;
            int vid[3];
            if (!cov_face(z, id[k], faces, vid)) continue;
            if (temp == 0.0f) { c[k] = code[k] == 0 ? 1.0f : 0.0f; continue; }   // no clip is evaluated
            AAFace a;
            cov_tables(im, vid, a);
            float area;
            const int err = tri_pix_overlap_area_only(a, pxmin, pxmax, pymin, pymax, pix_area, area);
            if (err != 0 || area == 0.0f) continue;
            c[k] = mix_coverage(code[k], area / pix_area, temp);         // forward.cu:375-381; no mask: the slot taken as a hit
        }
        if (LVEC == 4) *reinterpret_cast<float4*>(out + s0 + l) = make_float4(c[0], c[1 % LVEC], c[2 % LVEC], c[3 % LVEC]);
        else out[s0 + l] = c[0];
    }
}

// g_image (B,P,2) zero-filled by the caller.  A slot takes part when it is not empty, its upstream gradient is not zero, the
// clipper reports no error and a non-zero area, and the Jacobian is not all zero (full cover).  The ids are read one at a time:
// the clip and its Jacobian are inlined once, and a slot's 4 bytes are nothing next to them.
__global__ void __launch_bounds__(TILE_PIX)
k_coverage_bwd(CovSizes z, const int32_t* __restrict__ patch_min, const int32_t* __restrict__ layers, const float* __restrict__ image, const int32_t* __restrict__ faces,
               const float* __restrict__ g_cov, float* __restrict__ g_image) {
    __shared__ FaceTable<float, 6, LC_SLOTS + 6> tab;      // component 2 * vertex + (x, y); flush: bank = (6 c + slot) % 32
    const int tid = threadIdx.x;
    tab.clear(tid);
    __syncthreads();
    const auto [px, py, inside, pix] = tile_pixel(tid, z.W, z.H);
    const int b = blockIdx.z;
    float* gi = g_image + (int64_t)b * z.P * 2;
    const WinOrigin org = window_origin(patch_min);
    if (inside) {
        const int64_t s0 = pix * z.L;
        const float2* im = reinterpret_cast<const float2*>(image) + (int64_t)b * z.P;
        const float pxmin = (float)(px + org.x), pxmax = pxmin + 1, pymin = (float)(py + org.y), pymax = pymin + 1;
#pragma unroll 1
        for (int l = 0; l < z.L; l++) {
            const int f = layers[s0 + l];
            int vid[3];
            if (!cov_face(z, f, faces, vid)) continue;
            const float g = g_cov[s0 + l];
            if (g == 0.0f) continue;
            AAFace a;
            const bool flip = cov_tables(im, vid, a);
            float area, J[6];
            const int err = tri_pix_overlap_area<true>(a, pxmin, pxmax, pymin, pymax, 1.0f, area, J);
            if (err != 0 || area == 0.0f) continue;
            if (J[0] == 0.0f && J[1] == 0.0f && J[2] == 0.0f && J[3] == 0.0f && J[4] == 0.0f && J[5] == 0.0f) continue;
            const float s = g * z.temp;
            // corner k of the reordered triangle is vertex k of the face, 1 and 2 exchanged where the reorder swapped
            const float d[6] = {s * J[0], s * J[1], s * (flip ? J[4] : J[2]), s * (flip ? J[5] : J[3]),
                                s * (flip ? J[2] : J[4]), s * (flip ? J[3] : J[5])};
            const int slot = tab.slot(f);
#pragma unroll
            for (int j = 0; j < 6; j++) {
                if (d[j] == 0.0f) continue;
                if (slot >= 0) tab.add(slot, j, d[j]);
                else atomicAdd(gi + 2 * (int64_t)vid[j >> 1] + (j & 1), d[j]);
            }
        }
    }
    __syncthreads();
    // flush: one global atomic per (vertex row, component) and face of the tile (keys are listed, non-empty faces only)
    tab.flush_by_slot(tid, [&](int f, int j, float v) {
        atomicAdd(gi + 2 * (int64_t)faces[3 * (int64_t)f + (j >> 1)] + (j & 1), v);
    });
}

static CovSizes cov_sizes(int B, int H, int W, int L, int P, int F, float temperature) {
    CovSizes z;
    z.B = B; z.H = H; z.W = W; z.L = L; z.P = P; z.F = F; z.temp = temperature;
    return z;
}

void launch_coverage(int B, int H, int W, int L, int P, int F, float temperature, const int32_t* patch_min, const int32_t* render_layers,
                     const uint8_t* inside, const float* verts_image, const int32_t* faces, float* out_cov, hipStream_t st) {
    const CovSizes z = cov_sizes(B, H, W, L, P, F, temperature);
    const dim3 grid = tile_grid(W, H, B);
    const bool lvec = L % 4 == 0 && (((uintptr_t)render_layers | (uintptr_t)out_cov) & 15) == 0 && ((uintptr_t)inside & 3) == 0;
#define DM2_COV_LAUNCH(LVEC, MASK) \
    hipLaunchKernelGGL((k_coverage<LVEC, MASK>), grid, dim3(TILE_PIX), 0, st, z, patch_min, render_layers, inside, verts_image, faces, out_cov)
    if (lvec && inside) DM2_COV_LAUNCH(4, true);
    else if (lvec) DM2_COV_LAUNCH(4, false);
    else if (inside) DM2_COV_LAUNCH(1, true);
    else DM2_COV_LAUNCH(1, false);
#undef DM2_COV_LAUNCH
}

void launch_coverage_backward(int B, int H, int W, int L, int P, int F, float temperature, const int32_t* patch_min, const int32_t* render_layers,
                              const float* verts_image, const int32_t* faces, const float* dL_dcov, float* dL_dverts_image,
                              hipStream_t st) {
    const CovSizes z = cov_sizes(B, H, W, L, P, F, temperature);
    const dim3 grid = tile_grid(W, H, B);
    hipLaunchKernelGGL(k_coverage_bwd, grid, dim3(TILE_PIX), 0, st, z, patch_min, render_layers, verts_image, faces, dL_dcov, dL_dverts_image);
}

}  // namespace dm2
