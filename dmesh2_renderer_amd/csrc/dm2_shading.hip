// dm2_shading.hip -- Renderer.shading_vectors: the vectors a shader needs per slot s = (b, y, x, l), from rasterize's t, the
// pixel's own ray and interpolate's normal (include/dm2_hip.h: dm2_shading_vectors_window):
//   k_shading_vectors       position = ro + t rd,  view = -rd,  normal = n / |n|,  reflection = (2 (normal . view)) normal - view
//   k_shading_vectors_bwd   dL/dt = g_position . rd,  dL/dnormals = (G - normal (normal . G)) / |n| with
//                           G = g_normal + 2 c g_reflection + 2 (g_reflection . normal) view
//
// The ray is the one rasterize used: pixel_ray (dm2_stage.h) on the op's ray tensors or, under DM2_FLAG_ANALYTIC_RAYS, on the
// camera block at the absolute pixel of the window's frame.  One lane per slot, the view on blockIdx.z (the camera block and
// the window's origin are wave-uniform), rows of 12 bytes in and out: per slot 8 bytes (id, t) + 12 (normal) + the ray's 24
// shared by the pixel's L slots read, 24 or 48 written.  No LDS, no scratch, no atomics: every element of every output is
// written once, with a plain store.  -ffp-contract=off: the forward is a pure function of the written operation order
// (tests/shading_ref.py restates it).
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_stage.h"
#include "dm2_state.h"

namespace dm2 {

constexpr int SH_BLOCK = 256;

// what pixel_ray reads of an op's descriptor
struct ShadeRays {
    int flags;
    const float* ray_cam;
    const float* image_ray_o;
    const float* image_ray_d;
};

struct ShadeSizes {
    int64_t per_view;   // H * W * L
    int H, W, L, full_W, full_H;
};

__device__ __forceinline__ f3 sh_load3(const float* __restrict__ p, int64_t s) { return {p[3 * s], p[3 * s + 1], p[3 * s + 2]}; }
__device__ __forceinline__ void sh_store3(float* __restrict__ p, int64_t s, f3 v) { p[3 * s] = v.x; p[3 * s + 1] = v.y; p[3 * s + 2] = v.z; }
__device__ __forceinline__ float sh_dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// slot r of view blockIdx.z: false = empty (a negative id or a t that is not finite); else its ray
__device__ __forceinline__ bool sh_slot(const ShadeSizes& z, const ShadeRays& rays, const int32_t* __restrict__ patch_min, int64_t r,
                                        int64_t s, const int32_t* __restrict__ layers, const float* __restrict__ t, float& tt, f3& ro,
                                        f3& rd) {
    tt = t[s];
    if (layers[s] < 0 || !(fabsf(tt) < INFINITY)) return false;
    const int b = blockIdx.z;
    const int64_t pixel = r / z.L;
    const int y = (int)(pixel / z.W), x = (int)(pixel - (int64_t)y * z.W);
    const WinOrigin o = window_origin(patch_min);
    pixel_ray(rays, b, (int64_t)b * z.H * z.W + pixel, (uint32_t)x + o.x, (uint32_t)y + o.y, z.full_W, z.full_H, ro, rd);
    return true;
}

// normal = n / nl; false where nl is zero or not finite (a component that is not finite makes nl so)
__device__ __forceinline__ bool sh_normal(f3 n, f3& nrm, float& nl) {
    nl = sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
    if (!(nl < INFINITY) || nl == 0.0f) return false;
    nrm = {n.x / nl, n.y / nl, n.z / nl};
    return true;
}

__global__ void __launch_bounds__(SH_BLOCK)
k_shading_vectors(ShadeSizes z, ShadeRays rays, const int32_t* __restrict__ patch_min, const int32_t* __restrict__ layers,
                  const float* __restrict__ t, const float* __restrict__ normals, float* __restrict__ out_pos,
                  float* __restrict__ out_view, float* __restrict__ out_nrm, float* __restrict__ out_refl) {
    const int64_t r = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
    if (r >= z.per_view) return;
    const int64_t s = (int64_t)blockIdx.z * z.per_view + r;
    const f3 zero = {0.0f, 0.0f, 0.0f};
    f3 pos = zero, view = zero, nrm = zero, refl = zero, ro, rd;
    float tt;
    if (sh_slot(z, rays, patch_min, r, s, layers, t, tt, ro, rd)) {
        pos = {ro.x + tt * rd.x, ro.y + tt * rd.y, ro.z + tt * rd.z};
        view = -rd;
        if (normals) {
            f3 nn;
            float nl;
            if (sh_normal(sh_load3(normals, s), nn, nl)) {
                const float c = sh_dot(nn, view);
                const float c2 = 2.0f * c;
                nrm = nn;
                refl = {c2 * nn.x - view.x, c2 * nn.y - view.y, c2 * nn.z - view.z};
            }
        }
    }
    sh_store3(out_pos, s, pos);
    sh_store3(out_view, s, view);
    if (normals) {
        sh_store3(out_nrm, s, nrm);
        sh_store3(out_refl, s, refl);
    }
}

// g_pos, g_nrm, g_refl: NULL = that output was left out of the loss (zeros); dL_dt, dL_dn: NULL = not wanted
__global__ void __launch_bounds__(SH_BLOCK)
k_shading_vectors_bwd(ShadeSizes z, ShadeRays rays, const int32_t* __restrict__ patch_min, const int32_t* __restrict__ layers,
                      const float* __restrict__ t, const float* __restrict__ normals, const float* __restrict__ g_pos,
                      const float* __restrict__ g_nrm, const float* __restrict__ g_refl, float* __restrict__ dL_dt,
                      float* __restrict__ dL_dn) {
    const int64_t r = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
    if (r >= z.per_view) return;
    const int64_t s = (int64_t)blockIdx.z * z.per_view + r;
    const f3 zero = {0.0f, 0.0f, 0.0f};
    f3 dn = zero, ro, rd;
    float dt = 0.0f, tt;
    if (sh_slot(z, rays, patch_min, r, s, layers, t, tt, ro, rd)) {
        if (dL_dt && g_pos) dt = sh_dot(sh_load3(g_pos, s), rd);
        if (dL_dn) {
            f3 nn;
            float nl;
            if (sh_normal(sh_load3(normals, s), nn, nl)) {
                const f3 view = -rd;
                const f3 gn = g_nrm ? sh_load3(g_nrm, s) : zero;
                const f3 gr = g_refl ? sh_load3(g_refl, s) : zero;
                const float c2 = 2.0f * sh_dot(nn, view), k2 = 2.0f * sh_dot(gr, nn);
                const f3 G = {(gn.x + c2 * gr.x) + k2 * view.x, (gn.y + c2 * gr.y) + k2 * view.y, (gn.z + c2 * gr.z) + k2 * view.z};
                const float nG = sh_dot(nn, G);
                dn = {(G.x - nn.x * nG) / nl, (G.y - nn.y * nG) / nl, (G.z - nn.z * nG) / nl};
            }
        }
    }
    if (dL_dt) dL_dt[s] = dt;
    if (dL_dn) sh_store3(dL_dn, s, dn);
}

static ShadeSizes sh_sizes(int H, int W, int L, int full_W, int full_H) {
    ShadeSizes z;
    z.per_view = (int64_t)H * W * L;
    z.H = H; z.W = W; z.L = L; z.full_W = full_W; z.full_H = full_H;
    return z;
}
static dim3 sh_grid(const ShadeSizes& z, int B) { return dim3((unsigned)((z.per_view + SH_BLOCK - 1) / SH_BLOCK), 1, (unsigned)B); }

// B * H * W * L > 0.  H, W: the arrays' own extents; full_W, full_H: the frame of the cameras; patch_min as for launch_coverage
void launch_shading_vectors(int B, int H, int W, int L, int flags, int full_W, int full_H, const int32_t* patch_min,
                            const int32_t* render_layers, const float* t, const float* normals, const float* image_ray_o,
                            const float* image_ray_d, const float* ray_cam, float* out_position, float* out_view, float* out_normal,
                            float* out_reflection, hipStream_t st) {
    const ShadeSizes z = sh_sizes(H, W, L, full_W, full_H);
    const ShadeRays rays = {flags, ray_cam, image_ray_o, image_ray_d};
    hipLaunchKernelGGL(k_shading_vectors, sh_grid(z, B), dim3(SH_BLOCK), 0, st, z, rays, patch_min, render_layers, t, normals,
                       out_position, out_view, out_normal, out_reflection);
}

void launch_shading_vectors_backward(int B, int H, int W, int L, int flags, int full_W, int full_H, const int32_t* patch_min,
                                     const int32_t* render_layers, const float* t, const float* normals, const float* image_ray_o,
                                     const float* image_ray_d, const float* ray_cam, const float* g_position, const float* g_normal,
                                     const float* g_reflection, float* dL_dt, float* dL_dnormals, hipStream_t st) {
    const ShadeSizes z = sh_sizes(H, W, L, full_W, full_H);
    const ShadeRays rays = {flags, ray_cam, image_ray_o, image_ray_d};
    hipLaunchKernelGGL(k_shading_vectors_bwd, sh_grid(z, B), dim3(SH_BLOCK), 0, st, z, rays, patch_min, render_layers, t, normals,
                       g_position, g_normal, g_reflection, dL_dt, dL_dnormals);
}

}  // namespace dm2
