// dm2_cov_tables.h -- the six AA tables of one projected triangle, built in registers from its three image corners the way
// pack_face builds them under DM2_FLAG_TABLES_FROM_IMAGE (dm2_stage.h; bit-identical to the fused host prep's k_aa_tables).
// Shared by the kernels that clip a listed face against its pixel without a staged AAFace: k_coverage, k_coverage_bwd
// (dm2_coverage.hip) and k_rasterize_overlap (dm2_rasterize.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"

namespace dm2 {

// whether the CCW reorder swaps corners 1 and 2 (pyrenderer.py:521-535): the triangle is clockwise
__device__ __forceinline__ bool cov_flip(float2 p0, float2 p1, float2 p2) {
    const float area2 = 0.5f * ((p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y));
    return area2 < 0.0f;
}

// The AA tables of the triangle with image corners p0, p1, p2.  Returns whether the CCW reorder swapped corners 1 and 2.
__device__ __forceinline__ bool cov_tables_pts(float2 p0, float2 p1, float2 p2, AAFace& a) {
    const bool flip = cov_flip(p0, p1, p2);
    const float2 q[3] = {p0, flip ? p2 : p1, flip ? p1 : p2};
    uint32_t zm = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float2 sv = q[i], ev = q[(i + 1) % 3];
        const float ex = ev.x - sv.x, ey = ev.y - sv.y;
        const float nx = -ey, ny = ex;
        a.v[2 * i] = sv.x; a.v[2 * i + 1] = sv.y;
        a.e[2 * i] = ex; a.e[2 * i + 1] = ey;
        a.r[2 * i] = 1.0f / ex; a.r[2 * i + 1] = 1.0f / ey;
        a.n[2 * i] = nx; a.n[2 * i + 1] = ny;
        a.c[i] = nx * sv.x + ny * sv.y;
        zm |= (fabsf(ex) < 1e-3f ? 1u : 0u) << (2 * i);
        zm |= (fabsf(ey) < 1e-3f ? 1u : 0u) << (2 * i + 1);
    }
    a.zmask = zm;
    a.bb[0] = fminf(fminf(a.v[0], a.v[2]), a.v[4]);
    a.bb[1] = fmaxf(fmaxf(a.v[0], a.v[2]), a.v[4]);
    a.bb[2] = fminf(fminf(a.v[1], a.v[3]), a.v[5]);
    a.bb[3] = fmaxf(fmaxf(a.v[1], a.v[3]), a.v[5]);
    return flip;
}

// The AA tables of the face with vertices vid in view `im`.
__device__ __forceinline__ bool cov_tables(const float2* __restrict__ im, const int vid[3], AAFace& a) {
    return cov_tables_pts(im[vid[0]], im[vid[1]], im[vid[2]], a);
}

}  // namespace dm2
