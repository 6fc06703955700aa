// dm2_bary_derivatives.hip -- Renderer.bary_derivatives: the footprint of a pixel on each listed face, per slot s = (b, y, x, l):
//   k_bary_derivatives   dbary_dx[s] = d(1 - u - v, u, v)/dX,  dbary_dy[s] = d(1 - u - v, u, v)/dY   (X, Y: the pixel position in pixels)
//
// Contract (include/dm2_hip.h, dm2_bary_derivatives_window).  The unnormalised direction of analytic_ray (dm2_device_math.h),
// D = w - ro, is affine in the pixel position and u, v do not change when D is scaled, so with T = ro - p0, E1 = p1 - p0,
// E2 = p2 - p0, a = E2 x T, b = T x E1, c = E2 x E1:  u = D.a / D.c,  v = D.b / D.c, and for an axis with constant g = dD/dX
//   du/dX = (g.a - u (g.c)) / D.c     dv/dX = (g.b - v (g.c)) / D.c     d(bary0)/dX = -(du/dX + dv/dX).
// The kernel recomputes D, u, v from the camera block: it reads neither ray tensors nor rasterize's bary.  -ffp-contract=off:
// the result is a pure function of the written operation order.
//
// One lane per slot, the view on blockIdx.z (so the camera block, the two constant vectors g and the window's origin are
// wave-uniform), two 12-byte rows out.  Per slot: one face row, three vertices (36 bytes gathered), 24 bytes stored.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_state.h"

namespace dm2 {

constexpr int BD_BLOCK = 256;

__global__ void __launch_bounds__(BD_BLOCK)
k_bary_derivatives(int64_t per_view, int H, int W, int L, int P, int F, float Wf, float Hf, const int32_t* __restrict__ patch_min,
                   const int32_t* __restrict__ layers, const float* __restrict__ verts, const int32_t* __restrict__ faces,
                   const float* __restrict__ ray_cam, float* __restrict__ dbary_dx, float* __restrict__ dbary_dy) {
    const int64_t r = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
    if (r >= per_view) return;
    const int b = blockIdx.z;
    const int64_t s = (int64_t)b * per_view + r;
    const int64_t pixel = r / L;
    const int y = (int)(pixel / W), x = (int)(pixel - (int64_t)y * W);
    float ox[3] = {0.0f, 0.0f, 0.0f}, oy[3] = {0.0f, 0.0f, 0.0f};
    const int f = layers[s];
    if (f >= 0 && f < F) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if (i0 >= 0 && i0 < P && i1 >= 0 && i1 < P && i2 >= 0 && i2 < P) {
            const WinOrigin o = window_origin(patch_min);
            const float* imv = ray_cam + 32 * (int64_t)b;
            const float* ipr = imv + 16;
            // D = w - ro: analytic_ray's operations up to the normalisation
            const float xa = (float)(o.x + (uint32_t)x), ya = (float)(o.y + (uint32_t)y);
            const float h[4] = {((xa + 0.5f) / Wf * 2.0f) - 1.0f, ((ya + 0.5f) / Hf * 2.0f) - 1.0f, -1.0f, 1.0f};
            float v4[4], w3[3], gx[3], gy[3];
#pragma unroll
            for (int j = 0; j < 4; j++) v4[j] = ((h[0] * ipr[4 * j] + h[1] * ipr[4 * j + 1]) + h[2] * ipr[4 * j + 2]) + h[3] * ipr[4 * j + 3];
#pragma unroll
            for (int j = 0; j < 3; j++) w3[j] = ((v4[0] * imv[4 * j] + v4[1] * imv[4 * j + 1]) + v4[2] * imv[4 * j + 2]) + v4[3] * imv[4 * j + 3];
            const f3 ro = {imv[3], imv[7], imv[11]};
            const f3 D = {w3[0] - ro.x, w3[1] - ro.y, w3[2] - ro.z};
            // g = dD/dX, dD/dY: gX[k] = (2 / W) sum_j imv[4k+j] ipr[4j], gY[k] = (2 / H) sum_j imv[4k+j] ipr[4j+1]
            const float sx = 2.0f / Wf, sy = 2.0f / Hf;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                gx[k] = sx * (((imv[4 * k] * ipr[0] + imv[4 * k + 1] * ipr[4]) + imv[4 * k + 2] * ipr[8]) + imv[4 * k + 3] * ipr[12]);
                gy[k] = sy * (((imv[4 * k] * ipr[1] + imv[4 * k + 1] * ipr[5]) + imv[4 * k + 2] * ipr[9]) + imv[4 * k + 3] * ipr[13]);
            }
            const f3 gX = {gx[0], gx[1], gx[2]}, gY = {gy[0], gy[1], gy[2]};
            const f3 p0 = {verts[3 * i0], verts[3 * i0 + 1], verts[3 * i0 + 2]};
            const f3 p1 = {verts[3 * i1], verts[3 * i1 + 1], verts[3 * i1 + 2]};
            const f3 p2 = {verts[3 * i2], verts[3 * i2 + 1], verts[3 * i2 + 2]};
            const f3 T = ro - p0, E1 = p1 - p0, E2 = p2 - p0;
            const f3 a = cross(E2, T), bb = cross(T, E1), c = cross(E2, E1);
            const float Dc = dot(D, c);
            if (Dc != 0.0f) {
                const float rc = 1.0f / Dc;                                   // the one reciprocal
                const float u = dot(D, a) * rc, v = dot(D, bb) * rc;
                const float gcx = dot(gX, c), gcy = dot(gY, c);
                ox[1] = (dot(gX, a) - u * gcx) * rc;
                ox[2] = (dot(gX, bb) - v * gcx) * rc;
                ox[0] = -(ox[1] + ox[2]);
                oy[1] = (dot(gY, a) - u * gcy) * rc;
                oy[2] = (dot(gY, bb) - v * gcy) * rc;
                oy[0] = -(oy[1] + oy[2]);
            }
        }
    }
    float* dx = dbary_dx + 3 * s;
    float* dy = dbary_dy + 3 * s;
    dx[0] = ox[0]; dx[1] = ox[1]; dx[2] = ox[2];
    dy[0] = oy[0]; dy[1] = oy[1]; dy[2] = oy[2];
}

// win_W, win_H: the (B,H,W,L) arrays' own extents; full_W, full_H: the frame the cameras belong to
void launch_bary_derivatives(int B, int H, int W, int L, int P, int F, int full_W, int full_H, const int32_t* patch_min,
                             const int32_t* render_layers, const float* verts, const int32_t* faces, const float* ray_cam,
                             float* dbary_dx, float* dbary_dy, hipStream_t st) {
    const int64_t per_view = (int64_t)H * W * L;
    const dim3 grid((unsigned)((per_view + BD_BLOCK - 1) / BD_BLOCK), 1, (unsigned)B);
    hipLaunchKernelGGL(k_bary_derivatives, grid, dim3(BD_BLOCK), 0, st, per_view, H, W, L, P, F, (float)full_W, (float)full_H,
                       patch_min, render_layers, verts, faces, ray_cam, dbary_dx, dbary_dy);
}

}  // namespace dm2
