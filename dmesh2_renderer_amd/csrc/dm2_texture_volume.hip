// dm2_texture_volume.hip -- Renderer.texture3d: a channel-last voxel grid (N, N, N, C), indexed [k][j][i], looked up by a
// position (x, y, z) in its unit cube per slot s = (b, y, x, l):
//   k_texture_volume          out[s, c] = a0 + fz (a1 - a0), a_r the bilinear blend of plane k0 + r's four taps (nearest: one voxel)
//   k_texture_volume_bwd_xyz  dL/dxyz[s] = N (su0 + fz (su1 - su0), sv0 + fz (sv1 - sv0), sum_c g (a1 - a0)), su_r, sv_r the
//                             uv terms (tex_uv_term) of plane r
//   k_texture_volume_bwd_grid dL/dgrid[t_pqr, c] += w_pqr g[s, c]
//
// Contract (include/dm2_hip.h, dm2_texture_cube_backward, "DM2_TEX_VOLUME_*"): X = x N - 0.5 in fp32 (voxel centres at
// (i + 0.5) / N), X0 = floor(X), fx = X - X0, Y and Z alike; a slot is empty when its id is negative or |X|, |Y| or |Z| is not
// below 2^24 (NaN and infinite coordinates included): zeros out, nothing read from the grid through it, no gradient.
// -ffp-contract=off: the forward is a pure function of the written operation order.
//
// The kernels have the shapes of dm2_texture.hip's, for the reasons given there.  The forward stages one slot per lane in LDS:
// the flat index of tap (0, 0, 0), the three fractions and, per axis, the signed step from the axis' first tap to its second
// (0 where clamp folds both onto one voxel, negative where wrap returns to 0), so the eight taps are sums of one base and three
// steps; then dm2_tex_core.h's sweep, consecutive lanes on consecutive floats.  The position backward is one lane per slot.  The
// grid scatter is one block per 16 x 16 pixel tile and view, one layer at a time, through the block's table keyed by the flat
// voxel index with the eight (key, weight) pairs of tex_scatter_layer_masked.  A surface crosses a tile's voxels in a sheet:
// at N = 64 over a 1024-pixel frame a tile's layer touches a few dozen voxels; unrelated positions in a large grid overflow
// the table and go straight to global memory, as in the 2D op under minification.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"
#include "dm2_tex_core.h"

namespace dm2 {

struct VolSizes {
    int64_t S;        // B * H * W * L slots
    int64_t per_view; // slots per view (H * W * L)
    int64_t texels;   // N * N * N (< 2^31)
    int B, H, W, L, N, C;
    int view_textures; // grid is (B, N, N, N, C): voxel t of view b is voxel b * N * N * N + t
};

// one slot's sample: the flat index (k N + j) N + i of tap (0, 0, 0), the steps to the second tap of each axis, the fractions
// (nearest: idx alone, the steps and fractions 0)
struct VolTap {
    int idx, dx, dy, dz;
    float fx, fy, fz;
};

// false = empty slot (nothing of ``tap`` is set)
template <int FILTER, int BOUNDARY>
__device__ __forceinline__ bool vol_tap(const VolSizes& z, int64_t s, const int32_t* __restrict__ layers,
                                        const float* __restrict__ xyz, VolTap& tap) {
    if (layers && layers[s] < 0) return false;
    const int N = z.N;
    const float fn = (float)N;
    const float x = xyz[3 * s] * fn - 0.5f, y = xyz[3 * s + 1] * fn - 0.5f, w = xyz[3 * s + 2] * fn - 0.5f;
    if (!(fabsf(x) < TEX_RANGE) || !(fabsf(y) < TEX_RANGE) || !(fabsf(w) < TEX_RANGE)) return false;   // NaN and infinities included
    if (FILTER == TEX_NEAREST) {
        const int i = tex_addr<BOUNDARY>((int)floorf(x + 0.5f), N), j = tex_addr<BOUNDARY>((int)floorf(y + 0.5f), N);
        const int k = tex_addr<BOUNDARY>((int)floorf(w + 0.5f), N);
        tap.idx = (k * N + j) * N + i;
        tap.dx = tap.dy = tap.dz = 0;
        tap.fx = tap.fy = tap.fz = 0.0f;
        return true;
    }
    const float x0 = floorf(x), y0 = floorf(y), w0 = floorf(w);
    tap.fx = x - x0; tap.fy = y - y0; tap.fz = w - w0;
    const int i0 = (int)x0, j0 = (int)y0, k0 = (int)w0;
    const int ia = tex_addr<BOUNDARY>(i0, N), ja = tex_addr<BOUNDARY>(j0, N), ka = tex_addr<BOUNDARY>(k0, N);
    tap.idx = (ka * N + ja) * N + ia;
    tap.dx = tex_addr<BOUNDARY>(i0 + 1, N) - ia;
    tap.dy = (tex_addr<BOUNDARY>(j0 + 1, N) - ja) * N;
    tap.dz = (tex_addr<BOUNDARY>(k0 + 1, N) - ka) * N * N;
    return true;
}

template <int FILTER, int BOUNDARY, bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_volume(VolSizes z, const int32_t* __restrict__ layers, const float* __restrict__ xyz, const float* __restrict__ grid,
                 float* __restrict__ out) {
    __shared__ int s_idx[TEX_BLOCK];                                           // < 0: empty slot
    __shared__ int s_dx[TEX_BLOCK], s_dy[TEX_BLOCK], s_dz[TEX_BLOCK];          // (linear only: nearest stages the index alone)
    __shared__ float s_fx[TEX_BLOCK], s_fy[TEX_BLOCK], s_fz[TEX_BLOCK];
    __shared__ int s_view[TEX_BLOCK];
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * TEX_BLOCK;
    const int nslots = (int)min((int64_t)TEX_BLOCK, z.S - s0);
    if (tid < nslots) {
        const int64_t s = s0 + tid;
        VolTap tap;
        const bool ok = vol_tap<FILTER, BOUNDARY>(z, s, layers, xyz, tap);
        s_idx[tid] = ok ? tap.idx : -1;
        if (FILTER == TEX_LINEAR) {
            s_dx[tid] = ok ? tap.dx : 0; s_dy[tid] = ok ? tap.dy : 0; s_dz[tid] = ok ? tap.dz : 0;
            s_fx[tid] = ok ? tap.fx : 0.0f; s_fy[tid] = ok ? tap.fy : 0.0f; s_fz[tid] = ok ? tap.fz : 0.0f;
        }
        s_view[tid] = z.view_textures ? (int)(s / z.per_view) : 0;
    }
    __syncthreads();
    const int C = z.C;
    tex_sweep<VEC4>(tid, nslots, C, s_idx, out, s0, [&](int slot, int i000, int c) -> TexQuad {
        const float* p000 = grid + ((int64_t)s_view[slot] * z.texels + i000) * C + (int64_t)c * (VEC4 ? 4 : 1);
        if (FILTER == TEX_NEAREST) return tex_load_row<VEC4>(p000);
        const int64_t dx = (int64_t)s_dx[slot] * C, dy = (int64_t)s_dy[slot] * C, dz = (int64_t)s_dz[slot] * C;
        const float fx = s_fx[slot], fy = s_fy[slot], fz = s_fz[slot];
        const float* p001 = p000 + dz;
        const TexQuad a0 = tex_sample_rows<VEC4>(p000, p000 + dx, p000 + dy, p000 + dy + dx, fx, fy);
        const TexQuad a1 = tex_sample_rows<VEC4>(p001, p001 + dx, p001 + dy, p001 + dy + dx, fx, fy);
        if (VEC4) return {a0.x + fz * (a1.x - a0.x), a0.y + fz * (a1.y - a0.y), a0.z + fz * (a1.z - a0.z), a0.w + fz * (a1.w - a0.w)};
        return {a0.x + fz * (a1.x - a0.x), 0.0f, 0.0f, 0.0f};
    });
}

// one channel's terms of the position backward: the uv terms of both planes and g (a1 - a0)
struct VolSums { float su0, sv0, su1, sv1, sw; };
__device__ __forceinline__ void vol_xyz_term(float t000, float t100, float t010, float t110, float t001, float t101, float t011,
                                             float t111, float g, float fx, float fy, VolSums& m) {
    tex_uv_term(t000, t100, t010, t110, g, fx, fy, m.su0, m.sv0);
    tex_uv_term(t001, t101, t011, t111, g, fx, fy, m.su1, m.sv1);
    m.sw += g * (tex_bilinear(t001, t101, t011, t111, fx, fy) - tex_bilinear(t000, t100, t010, t110, fx, fy));
}

// (linear only: the entry point zero-fills dL_dxyz for nearest.)  The sums run over the channels in the same order on the
// VEC4 path.
template <int BOUNDARY, bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_volume_bwd_xyz(VolSizes z, const int32_t* __restrict__ layers, const float* __restrict__ xyz, const float* __restrict__ grid,
                         const float* __restrict__ g, float* __restrict__ dL_dxyz) {
    const int64_t s = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (s >= z.S) return;
    VolTap tap;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (vol_tap<TEX_LINEAR, BOUNDARY>(z, s, layers, xyz, tap)) {
        const int C = z.C;
        const int64_t dx = (int64_t)tap.dx * C, dy = (int64_t)tap.dy * C, dz = (int64_t)tap.dz * C;
        const float* p000 = grid + ((z.view_textures ? (s / z.per_view) * z.texels : 0) + tap.idx) * C;
        const float* p100 = p000 + dx;
        const float* p010 = p000 + dy;
        const float* p110 = p010 + dx;
        const float* p001 = p000 + dz;
        const float* p101 = p001 + dx;
        const float* p011 = p001 + dy;
        const float* p111 = p011 + dx;
        const float* gs = g + s * C;
        const float fx = tap.fx, fy = tap.fy;
        VolSums m = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (VEC4) {
            for (int c = 0; c < C; c += 4) {
                const float4 t000 = *reinterpret_cast<const float4*>(p000 + c), t100 = *reinterpret_cast<const float4*>(p100 + c);
                const float4 t010 = *reinterpret_cast<const float4*>(p010 + c), t110 = *reinterpret_cast<const float4*>(p110 + c);
                const float4 t001 = *reinterpret_cast<const float4*>(p001 + c), t101 = *reinterpret_cast<const float4*>(p101 + c);
                const float4 t011 = *reinterpret_cast<const float4*>(p011 + c), t111 = *reinterpret_cast<const float4*>(p111 + c);
                const float4 gv = *reinterpret_cast<const float4*>(gs + c);
                vol_xyz_term(t000.x, t100.x, t010.x, t110.x, t001.x, t101.x, t011.x, t111.x, gv.x, fx, fy, m);
                vol_xyz_term(t000.y, t100.y, t010.y, t110.y, t001.y, t101.y, t011.y, t111.y, gv.y, fx, fy, m);
                vol_xyz_term(t000.z, t100.z, t010.z, t110.z, t001.z, t101.z, t011.z, t111.z, gv.z, fx, fy, m);
                vol_xyz_term(t000.w, t100.w, t010.w, t110.w, t001.w, t101.w, t011.w, t111.w, gv.w, fx, fy, m);
            }
        } else {
            for (int c = 0; c < C; c++) vol_xyz_term(p000[c], p100[c], p010[c], p110[c], p001[c], p101[c], p011[c], p111[c], gs[c], fx, fy, m);
        }
        const float fn = (float)z.N;
        gx = fn * (m.su0 + tap.fz * (m.su1 - m.su0));
        gy = fn * (m.sv0 + tap.fz * (m.sv1 - m.sv0));
        gz = fn * m.sw;
    }
    dL_dxyz[3 * s] = gx; dL_dxyz[3 * s + 1] = gy; dL_dxyz[3 * s + 2] = gz;
}

template <int FILTER, int BOUNDARY, int CH>
__global__ void __launch_bounds__(TILE_PIX)
k_texture_volume_bwd_grid(VolSizes z, const int32_t* __restrict__ layers, const float* __restrict__ xyz, const float* __restrict__ g,
                          float* __restrict__ dL_dgrid) {
    constexpr int NTAP = FILTER == TEX_LINEAR ? 8 : 1;
    __shared__ TexTable<CH> tab;
    const int b = blockIdx.z, tid = threadIdx.x;
    const TilePixel t = tile_pixel(tid, z.W, z.H);
    const int C = z.C, L = z.L;
    float* dst = dL_dgrid + (z.view_textures ? (int64_t)b * z.texels * C : 0);
    for (int l = 0; l < L; l++) {
        const int64_t s = t.pix * L + l;
        VolTap tap = {0, 0, 0, 0, 0.0f, 0.0f, 0.0f};
        const bool live = t.inside && vol_tap<FILTER, BOUNDARY>(z, s, layers, xyz, tap);
        // tap p + 2 q + 4 r: key base + p dx + q dy + r dz, weight (wx_p * wy_q) * wz_r
        int key[NTAP];
        float w[NTAP];
        if (FILTER == TEX_LINEAR) {
            const float wx[2] = {1.0f - tap.fx, tap.fx}, wy[2] = {1.0f - tap.fy, tap.fy}, wz[2] = {1.0f - tap.fz, tap.fz};
#pragma unroll
            for (int k = 0; k < NTAP; k++) {
                key[k] = tap.idx + ((k & 1) ? tap.dx : 0) + ((k & 2) ? tap.dy : 0) + ((k & 4) ? tap.dz : 0);
                w[k] = (wx[k & 1] * wy[(k >> 1) & 1]) * wz[(k >> 2) & 1];
            }
        } else {
            key[0] = tap.idx; w[0] = 1.0f;
        }
        tex_scatter_layer_masked<CH, NTAP, false>(tab, tid, live, key, w, (1u << NTAP) - 1u, 0u, g, s, C,
                                                  [&](int k) { return dst + (int64_t)k * C; });
    }
}

static VolSizes vol_sizes(int B, int H, int W, int L, int N, int C, int view_textures) {
    VolSizes z;
    tex_common_sizes(z, B, H, W, L, C, view_textures);
    z.texels = (int64_t)N * N * N;
    z.N = N;
    return z;
}

void launch_texture_volume(int B, int H, int W, int L, int N, int C, int view_textures, int filter, int boundary,
                           const int32_t* render_layers, const float* xyz, const float* grid, float* out, hipStream_t st) {
    const VolSizes z = vol_sizes(B, H, W, L, N, C, view_textures);
    const dim3 blocks = tex_flat_grid(z.S);
    const bool vec4 = C % 4 == 0 && tex_aligned16(grid, out);
#define DM2_VOL_FWD(F, Bd)                                                                                                                 \
    do {                                                                                                                                   \
        if (vec4) hipLaunchKernelGGL((k_texture_volume<F, Bd, true>), blocks, dim3(TEX_BLOCK), 0, st, z, render_layers, xyz, grid, out);    \
        else hipLaunchKernelGGL((k_texture_volume<F, Bd, false>), blocks, dim3(TEX_BLOCK), 0, st, z, render_layers, xyz, grid, out);        \
    } while (0)
    DM2_TEX_MODES(filter, boundary, DM2_VOL_FWD);
#undef DM2_VOL_FWD
}

void launch_texture_volume_backward(int B, int H, int W, int L, int N, int C, int view_textures, int filter, int boundary,
                                    const int32_t* render_layers, const float* xyz, const float* grid, const float* dL_dout,
                                    float* dL_dgrid, float* dL_dxyz, hipStream_t st) {
    const VolSizes z = vol_sizes(B, H, W, L, N, C, view_textures);
    if (dL_dxyz) {
        const dim3 blocks = tex_flat_grid(z.S);                             // (linear: the entry point zero-fills for nearest)
        const bool vec4 = C % 4 == 0 && tex_aligned16(grid, dL_dout);
#define DM2_VOL_XYZ(Bd, V4) hipLaunchKernelGGL((k_texture_volume_bwd_xyz<Bd, V4>), blocks, dim3(TEX_BLOCK), 0, st, z, render_layers, xyz, grid, dL_dout, dL_dxyz)
        if (boundary == TEX_WRAP) { if (vec4) DM2_VOL_XYZ(TEX_WRAP, true); else DM2_VOL_XYZ(TEX_WRAP, false); }
        else { if (vec4) DM2_VOL_XYZ(TEX_CLAMP, true); else DM2_VOL_XYZ(TEX_CLAMP, false); }
#undef DM2_VOL_XYZ
    }
    if (dL_dgrid) {
        const dim3 blocks = tile_grid(W, H, B);
#define DM2_VOL_GRID(F, Bd, CH) hipLaunchKernelGGL((k_texture_volume_bwd_grid<F, Bd, CH>), blocks, dim3(TILE_PIX), 0, st, z, render_layers, xyz, dL_dout, dL_dgrid)
#define DM2_VOL_GRID_MODES(F, Bd) DM2_TEX_CHUNK(C, DM2_VOL_GRID, F, Bd)
        DM2_TEX_MODES(filter, boundary, DM2_VOL_GRID_MODES);
#undef DM2_VOL_GRID_MODES
#undef DM2_VOL_GRID
    }
}

}  // namespace dm2
