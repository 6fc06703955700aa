// dm2_texture_cube.hip -- Renderer.texture(boundary_mode="cube"): a channel-last cube map (6, N, N, C) looked up by a direction
// per slot s = (b, y, x, l):
//   k_texture_cube          out[s, c] = a + fy (b - a) over four taps that may lie on the adjacent face; three taps with their
//                           weights renormalised at a cube corner; nearest: one texel
//   k_texture_cube_bwd_dir  dL/ddir[s] through fx, fy -> s, t -> sc / ma, tc / ma (zeros for nearest: the entry point fills them)
//   k_texture_cube_bwd_tex  dL/dtex[t_k, c] += w_k g[s, c]
//
// Contract (include/dm2_hip.h, dm2_texture_cube): the major axis picks the face, (sc, tc, ma) by the OpenGL table,
// s = 0.5 (sc / ma + 1), x = s N - 0.5 in [-0.5, N - 0.5], x0 = floor(x), fx = x - x0 (y alike); a slot is empty when its id is
// negative, a component of the direction is not finite, or all three are zero: zeros out, nothing read from tex through it,
// no gradient.  -ffp-contract=off: the forward is a pure function of the written operation order.
//
// The kernels have the shapes of dm2_texture.hip's, for the reasons given there: the forward stages one slot per lane in LDS
// (four flat texel indices face N N + j N + i, the fractions, the missing tap of a corner) and sweeps the block's 256 * C
// outputs with consecutive lanes on consecutive floats; the direction backward is one lane per slot; the texel scatter is one
// block per 16 x 16 pixel tile and view, one layer at a time, through the block's FaceTable keyed by the flat texel index.
// What is new is cube_tap(): the face selection, the seam rule for a tap beyond one border (CUBE_SEAM, a constant table read
// only by the lanes that have such a tap) and the corner flag; everything after it sees four addresses and two fractions, as
// the 2D op does, and takes them through the same code: the blend, the uv terms, the sweep and the scatter are
// dm2_tex_core.h's.  The corner sample (three taps, renormalised weights) and its gradient stay here.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_face_table.h"
#include "dm2_state.h"
#include "dm2_tex_core.h"

namespace dm2 {

// borders of a face: 0: i < 0 (s = 0), 1: i >= N (s = 1), 2: j < 0 (t = 0), 3: j >= N (t = 1).
// CUBE_SEAM[face][border] = {the face across that border, which of ITS borders the shared edge is, 1 when the position along
// the edge runs the other way there}; faces +x, -x, +y, -y, +z, -z.  (tests/texture_cube_ref.py derives it from the geometry.)
__device__ __constant__ signed char CUBE_SEAM[6][4][3] = {
    {{4, 1, 0}, {5, 0, 0}, {2, 1, 1}, {3, 1, 0}},
    {{5, 1, 0}, {4, 0, 0}, {2, 0, 0}, {3, 0, 1}},
    {{1, 2, 0}, {0, 2, 1}, {5, 2, 1}, {4, 2, 0}},
    {{1, 3, 1}, {0, 3, 0}, {4, 3, 0}, {5, 3, 1}},
    {{1, 1, 0}, {0, 0, 0}, {2, 3, 0}, {3, 2, 0}},
    {{0, 1, 0}, {1, 0, 0}, {2, 2, 1}, {3, 3, 1}},
};

struct CubeSizes {
    int64_t S;        // B * H * W * L slots
    int64_t per_view; // slots per view (H * W * L)
    int64_t texels;   // 6 * N * N (< 2^31)
    int B, H, W, L, N, C;
    int view_textures; // tex is (B, 6, N, N, C): texel t of view b is texel b * 6 * N * N + t
};

// one slot's sample: flat texel indices of the taps (t00, t10, t01, t11; nearest: idx[0] alone), the fractions, and the tap
// that does not exist at a cube corner (-1: all four exist; its idx is idx of an existing tap and is never used)
struct CubeTap {
    int idx[4];
    float fx, fy;
    int miss;
};

// the face and its coordinates; false = empty slot
struct CubeFace {
    int face;
    float sc, tc, ma;
};

__device__ __forceinline__ bool cube_face(const CubeSizes& z, int64_t s, const int32_t* __restrict__ layers,
                                          const float* __restrict__ dirs, CubeFace& f) {
    if (layers && layers[s] < 0) return false;
    const float x = dirs[3 * s], y = dirs[3 * s + 1], zz = dirs[3 * s + 2];
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(zz);
    if (!(ax < INFINITY) || !(ay < INFINITY) || !(az < INFINITY)) return false;      // NaN and infinities
    if (ax == 0.0f && ay == 0.0f && az == 0.0f) return false;
    if (ax >= ay && ax >= az) {
        const int neg = x < 0.0f;                                          // (the major component is not zero here)
        f.face = neg; f.ma = ax; f.sc = neg ? zz : -zz; f.tc = -y;
    } else if (ay >= az) {
        const int neg = y < 0.0f;
        f.face = 2 + neg; f.ma = ay; f.sc = x; f.tc = neg ? -zz : zz;
    } else {
        const int neg = zz < 0.0f;
        f.face = 4 + neg; f.ma = az; f.sc = neg ? -x : x; f.tc = -y;
    }
    return true;
}

// flat index of tap (i, j) of ``face`` after the seam rule; -1: beyond two borders (a cube corner)
__device__ __forceinline__ int cube_texel(int N, int face, int i, int j) {
    const bool ox = (unsigned)i >= (unsigned)N, oy = (unsigned)j >= (unsigned)N;
    if (ox || oy) {
        if (ox && oy) return -1;
        const int e = ox ? (i < 0 ? 0 : 1) : (j < 0 ? 2 : 3);
        const int k = ox ? j : i;
        const signed char* row = CUBE_SEAM[face][e];
        const int ne = row[1];
        const int kk = row[2] ? N - 1 - k : k;
        face = row[0];
        i = ne == 0 ? 0 : (ne == 1 ? N - 1 : kk);
        j = ne == 2 ? 0 : (ne == 3 ? N - 1 : kk);
    }
    return (face * N + j) * N + i;
}

// false = empty slot (nothing of ``tap`` or ``f`` is to be used)
template <int FILTER>
__device__ __forceinline__ bool cube_tap(const CubeSizes& z, int64_t s, const int32_t* __restrict__ layers,
                                         const float* __restrict__ dirs, CubeTap& tap, CubeFace& f) {
    if (!cube_face(z, s, layers, dirs, f)) return false;
    const int N = z.N;
    const float sn = 0.5f * (f.sc / f.ma + 1.0f), tn = 0.5f * (f.tc / f.ma + 1.0f);
    const float x = sn * (float)N - 0.5f, y = tn * (float)N - 0.5f;
    tap.miss = -1;
    if (FILTER == TEX_NEAREST) {
        const int i = min(max((int)floorf(x + 0.5f), 0), N - 1), j = min(max((int)floorf(y + 0.5f), 0), N - 1);
        tap.idx[0] = (f.face * N + j) * N + i;
        tap.idx[1] = tap.idx[2] = tap.idx[3] = tap.idx[0];
        tap.fx = tap.fy = 0.0f;
        return true;
    }
    const float x0 = floorf(x), y0 = floorf(y);
    tap.fx = x - x0; tap.fy = y - y0;
    // |sc / ma| <= 1 puts x0 in [-1, N - 1] by itself; the clamp keeps every address inside the cube whatever the division gave
    const int i0 = min(max((int)x0, -1), N - 1), j0 = min(max((int)y0, -1), N - 1);
    const int t0 = cube_texel(N, f.face, i0, j0), t1 = cube_texel(N, f.face, i0 + 1, j0);
    const int t2 = cube_texel(N, f.face, i0, j0 + 1), t3 = cube_texel(N, f.face, i0 + 1, j0 + 1);
    // at most one tap is missing (x0 in [-1, N - 1]); of each row of taps one is inside the face's columns
    tap.miss = t0 < 0 ? 0 : (t1 < 0 ? 1 : (t2 < 0 ? 2 : (t3 < 0 ? 3 : -1)));
    tap.idx[0] = t0 < 0 ? t3 : t0; tap.idx[1] = t1 < 0 ? t2 : t1; tap.idx[2] = t2 < 0 ? t1 : t2; tap.idx[3] = t3 < 0 ? t0 : t3;
    return true;
}

// the weights of a corner sample: w_miss = 0, W their sum in the written order
struct CornerW { float w0, w1, w2, w3, W; };
__device__ __forceinline__ CornerW cb_corner_w(float fx, float fy, int miss) {
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    CornerW c;
    c.w0 = miss == 0 ? 0.0f : gx * gy; c.w1 = miss == 1 ? 0.0f : fx * gy;
    c.w2 = miss == 2 ? 0.0f : gx * fy; c.w3 = miss == 3 ? 0.0f : fx * fy;
    c.W = ((c.w0 + c.w1) + c.w2) + c.w3;
    return c;
}

// (t_miss = 0: what was loaded for the missing tap is not used)
__device__ __forceinline__ float cb_corner(float t0, float t1, float t2, float t3, const CornerW& c, int miss) {
    t0 = miss == 0 ? 0.0f : t0; t1 = miss == 1 ? 0.0f : t1; t2 = miss == 2 ? 0.0f : t2; t3 = miss == 3 ? 0.0f : t3;
    return (((c.w0 * t0 + c.w1 * t1) + c.w2 * t2) + c.w3 * t3) / c.W;
}

template <int FILTER, bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_cube(CubeSizes z, const int32_t* __restrict__ layers, const float* __restrict__ dirs, const float* __restrict__ tex,
               float* __restrict__ out) {
    constexpr int NIDX = FILTER == TEX_LINEAR ? 4 : 1;
    __shared__ int s_idx[NIDX][TEX_BLOCK];                                     // idx[0] < 0: empty slot
    __shared__ float s_fx[TEX_BLOCK], s_fy[TEX_BLOCK];
    __shared__ int s_view[TEX_BLOCK];                                          // view * 8 + (miss + 1)
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * TEX_BLOCK;
    const int nslots = (int)min((int64_t)TEX_BLOCK, z.S - s0);
    if (tid < nslots) {
        const int64_t s = s0 + tid;
        CubeTap tap;
        CubeFace f;
        const bool ok = cube_tap<FILTER>(z, s, layers, dirs, tap, f);
#pragma unroll
        for (int k = 0; k < NIDX; k++) s_idx[k][tid] = ok ? tap.idx[k] : -1;
        s_fx[tid] = ok ? tap.fx : 0.0f; s_fy[tid] = ok ? tap.fy : 0.0f;
        s_view[tid] = (z.view_textures ? (int)(s / z.per_view) : 0) * 8 + (ok ? tap.miss + 1 : 0);
    }
    __syncthreads();
    const int C = z.C;
    tex_sweep<VEC4>(tid, nslots, C, s_idx[0], out, s0, [&](int slot, int i00, int c) -> TexQuad {
        const int vm = s_view[slot];
        const float* base = tex + (int64_t)(vm >> 3) * z.texels * C + (int64_t)c * (VEC4 ? 4 : 1);
        if (FILTER == TEX_NEAREST) return tex_load_row<VEC4>(base + (int64_t)i00 * C);
        const float fx = s_fx[slot], fy = s_fy[slot];
        const int miss = (vm & 7) - 1;
        const float* p00 = base + (int64_t)i00 * C;
        const float* p10 = base + (int64_t)s_idx[NIDX > 1 ? 1 : 0][slot] * C;
        const float* p01 = base + (int64_t)s_idx[NIDX > 1 ? 2 : 0][slot] * C;
        const float* p11 = base + (int64_t)s_idx[NIDX > 1 ? 3 : 0][slot] * C;
        if (!VEC4) {
            if (miss < 0) return tex_sample_rows<false>(p00, p10, p01, p11, fx, fy);
            return {cb_corner(*p00, *p10, *p01, *p11, cb_corner_w(fx, fy, miss), miss), 0.0f, 0.0f, 0.0f};
        }
        const TexQuad t00 = tex_load_row<VEC4>(p00), t10 = tex_load_row<VEC4>(p10), t01 = tex_load_row<VEC4>(p01), t11 = tex_load_row<VEC4>(p11);
        if (miss < 0) return tex_blend_rows<VEC4>(t00, t10, t01, t11, fx, fy);
        const CornerW cw = cb_corner_w(fx, fy, miss);
        return {cb_corner(t00.x, t10.x, t01.x, t11.x, cw, miss), cb_corner(t00.y, t10.y, t01.y, t11.y, cw, miss),
                cb_corner(t00.z, t10.z, t01.z, t11.z, cw, miss), cb_corner(t00.w, t10.w, t01.w, t11.w, cw, miss)};
    });
}

// the uv terms (tex_uv_term) at a corner: out = sum_k w_k t_k / W, d out / d fx = sum_k (dw_k / dfx) (t_k - out) / W (the 1 / W is applied to the sums)
struct CornerD { float x0, x1, x2, x3, y0, y1, y2, y3; };
__device__ __forceinline__ void cb_dir_term_corner(float t0, float t1, float t2, float t3, float g, const CornerW& cw, const CornerD& d,
                                                   int miss, float& su, float& sv) {
    const float o = cb_corner(t0, t1, t2, t3, cw, miss);
    const float r0 = t0 - o, r1 = t1 - o, r2 = t2 - o, r3 = t3 - o;       // (a missing tap's d is 0)
    su += g * (((d.x0 * r0 + d.x1 * r1) + d.x2 * r2) + d.x3 * r3);
    sv += g * (((d.y0 * r0 + d.y1 * r1) + d.y2 * r2) + d.y3 * r3);
}

// (linear only: the entry point zero-fills dL_ddir for nearest.)  VEC4 as in k_texture_cube: the sums run over the channels in
// the same order either way.
template <bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_cube_bwd_dir(CubeSizes z, const int32_t* __restrict__ layers, const float* __restrict__ dirs, const float* __restrict__ tex,
                       const float* __restrict__ g, float* __restrict__ dL_ddir) {
    const int64_t s = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (s >= z.S) return;
    CubeTap tap;
    CubeFace f;
    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    if (cube_tap<TEX_LINEAR>(z, s, layers, dirs, tap, f)) {
        const int C = z.C, miss = tap.miss;
        const float* base = tex + (z.view_textures ? (s / z.per_view) * z.texels * C : 0);
        const float* p00 = base + (int64_t)tap.idx[0] * C;
        const float* p10 = base + (int64_t)tap.idx[1] * C;
        const float* p01 = base + (int64_t)tap.idx[2] * C;
        const float* p11 = base + (int64_t)tap.idx[3] * C;
        const float* gs = g + s * C;
        const float fx = tap.fx, fy = tap.fy;
        float su = 0.0f, sv = 0.0f;
        if (miss < 0) {
            if (VEC4) {
                for (int c = 0; c < C; c += 4) {
                    const float4 t00 = *reinterpret_cast<const float4*>(p00 + c), t10 = *reinterpret_cast<const float4*>(p10 + c);
                    const float4 t01 = *reinterpret_cast<const float4*>(p01 + c), t11 = *reinterpret_cast<const float4*>(p11 + c);
                    const float4 gv = *reinterpret_cast<const float4*>(gs + c);
                    tex_uv_term(t00.x, t10.x, t01.x, t11.x, gv.x, fx, fy, su, sv);
                    tex_uv_term(t00.y, t10.y, t01.y, t11.y, gv.y, fx, fy, su, sv);
                    tex_uv_term(t00.z, t10.z, t01.z, t11.z, gv.z, fx, fy, su, sv);
                    tex_uv_term(t00.w, t10.w, t01.w, t11.w, gv.w, fx, fy, su, sv);
                }
            } else {
                for (int c = 0; c < C; c++) tex_uv_term(p00[c], p10[c], p01[c], p11[c], gs[c], fx, fy, su, sv);
            }
        } else {
            const CornerW cw = cb_corner_w(fx, fy, miss);
            const float gx = 1.0f - fx, gy = 1.0f - fy;
            CornerD d;
            d.x0 = miss == 0 ? 0.0f : -gy; d.x1 = miss == 1 ? 0.0f : gy; d.x2 = miss == 2 ? 0.0f : -fy; d.x3 = miss == 3 ? 0.0f : fy;
            d.y0 = miss == 0 ? 0.0f : -gx; d.y1 = miss == 1 ? 0.0f : -fx; d.y2 = miss == 2 ? 0.0f : gx; d.y3 = miss == 3 ? 0.0f : fx;
            // (the scalar loop on both paths: corners are a few slots of a frame, and the order of the sum is the same)
            for (int c = 0; c < C; c++) cb_dir_term_corner(p00[c], p10[c], p01[c], p11[c], gs[c], cw, d, miss, su, sv);
            su = su / cw.W; sv = sv / cw.W;
        }
        // x = s N - 0.5, s = 0.5 (u + 1), u = sc / ma
        const float A = 0.5f * (float)z.N * su, Bq = 0.5f * (float)z.N * sv;
        const float inv = 1.0f / f.ma;
        const float dsc = A * inv, dtc = Bq * inv, dma = -((A * f.sc + Bq * f.tc) * inv) * inv;
        const int neg = f.face & 1;
        const float dmaj = neg ? -dma : dma;
        if (f.face < 2) { dx = dmaj; dy = -dtc; dz = neg ? dsc : -dsc; }
        else if (f.face < 4) { dx = dsc; dy = dmaj; dz = neg ? -dtc : dtc; }
        else { dx = neg ? -dsc : dsc; dy = -dtc; dz = dmaj; }
    }
    dL_ddir[3 * s] = dx; dL_ddir[3 * s + 1] = dy; dL_ddir[3 * s + 2] = dz;
}

template <int FILTER, int CH>
__global__ void __launch_bounds__(TILE_PIX)
k_texture_cube_bwd_tex(CubeSizes z, const int32_t* __restrict__ layers, const float* __restrict__ dirs, const float* __restrict__ g,
                       float* __restrict__ dL_dtex) {
    constexpr int NTAP = FILTER == TEX_LINEAR ? 4 : 1;
    __shared__ TexTable<CH> tab;
    const int b = blockIdx.z, tid = threadIdx.x;
    const TilePixel t = tile_pixel(tid, z.W, z.H);
    const int C = z.C, L = z.L;
    float* dst = dL_dtex + (z.view_textures ? (int64_t)b * z.texels * C : 0);
    for (int l = 0; l < L; l++) {
        const int64_t s = t.pix * L + l;
        CubeTap tap = {{0, 0, 0, 0}, 0.0f, 0.0f, -1};
        CubeFace f;
        const bool live = t.inside && cube_tap<FILTER>(z, s, layers, dirs, tap, f);
        float w[4] = {(1.0f - tap.fx) * (1.0f - tap.fy), tap.fx * (1.0f - tap.fy), (1.0f - tap.fx) * tap.fy, tap.fx * tap.fy};
        if (tap.miss >= 0) {                                                  // a corner: the three weights over their sum
            const CornerW cw = cb_corner_w(tap.fx, tap.fy, tap.miss);
            w[0] = cw.w0 / cw.W; w[1] = cw.w1 / cw.W; w[2] = cw.w2 / cw.W; w[3] = cw.w3 / cw.W;
        }
        const float one[1] = {1.0f};
        tex_scatter_layer<CH, NTAP, false>(tab, tid, live, tap.idx, FILTER == TEX_LINEAR ? w : one, NTAP, tap.miss, g, s, C,
                                           [&](int key) { return dst + (int64_t)key * C; });    // (miss: no texel, its idx is another tap's)
    }
}

static CubeSizes cb_sizes(int B, int H, int W, int L, int N, int C, int view_textures) {
    CubeSizes z;
    tex_common_sizes(z, B, H, W, L, C, view_textures);
    z.texels = (int64_t)6 * N * N;
    z.N = N;
    return z;
}

void launch_texture_cube(int B, int H, int W, int L, int N, int C, int view_textures, int filter, const int32_t* render_layers,
                         const float* dirs, const float* tex, float* out, hipStream_t st) {
    const CubeSizes z = cb_sizes(B, H, W, L, N, C, view_textures);
    const dim3 grid = tex_flat_grid(z.S);
    const bool vec4 = C % 4 == 0 && tex_aligned16(tex, out);
#define DM2_CB_FWD(F, V4) hipLaunchKernelGGL((k_texture_cube<F, V4>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, dirs, tex, out)
    if (filter == TEX_LINEAR) { if (vec4) DM2_CB_FWD(TEX_LINEAR, true); else DM2_CB_FWD(TEX_LINEAR, false); }
    else { if (vec4) DM2_CB_FWD(TEX_NEAREST, true); else DM2_CB_FWD(TEX_NEAREST, false); }
#undef DM2_CB_FWD
}

void launch_texture_cube_backward(int B, int H, int W, int L, int N, int C, int view_textures, int filter,
                                  const int32_t* render_layers, const float* dirs, const float* tex, const float* dL_dout,
                                  float* dL_dtex, float* dL_ddir, hipStream_t st) {
    const CubeSizes z = cb_sizes(B, H, W, L, N, C, view_textures);
    if (dL_ddir) {
        const dim3 grid = tex_flat_grid(z.S);                               // (linear: the entry point zero-fills for nearest)
        if (C % 4 == 0 && tex_aligned16(tex, dL_dout))
            hipLaunchKernelGGL((k_texture_cube_bwd_dir<true>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, dirs, tex, dL_dout, dL_ddir);
        else
            hipLaunchKernelGGL((k_texture_cube_bwd_dir<false>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, dirs, tex, dL_dout, dL_ddir);
    }
    if (dL_dtex) {
        const dim3 grid = tile_grid(W, H, B);
#define DM2_CB_TEX(F, CH) hipLaunchKernelGGL((k_texture_cube_bwd_tex<F, CH>), grid, dim3(TILE_PIX), 0, st, z, render_layers, dirs, dL_dout, dL_dtex)
        if (filter == TEX_LINEAR) DM2_TEX_CHUNK(C, DM2_CB_TEX, TEX_LINEAR); else DM2_TEX_CHUNK(C, DM2_CB_TEX, TEX_NEAREST);
#undef DM2_CB_TEX
    }
}

// ---- the cube's mip chain: texture(filter_mode="linear-mipmap-linear", boundary_mode="cube", mip_level=...) ----
//   k_texture_cube_mip          out[s, c] = c_j + f (c_{j+1} - c_j), c_k = the linear cube sample of level k (one level where
//                               lod <= 0 or lod >= nlev - 1); lod is the slot's own, given by the caller
//   k_texture_cube_mip_bwd_dir  (dL/ddir, dL/dlod)[s] = ((1 - f) ddir_j + f ddir_{j+1}, sum_c g (c_{j+1} - c_j)), one 16-byte row
//   k_texture_cube_mip_bwd_tex  dL/dtex, dL/dmip[t of level j, j + 1] += (1 - f) w g, f w g
// Contract: include/dm2_hip.h, dm2_texture_cube_mip.  The face and (sc, tc, ma) are the slot's, computed
// once; each level repeats cube_tap's linear stage at its own size N_k = N >> k (cm_level).  A texel of any level has one key per
// view, as in dm2_texture_mip.hip: level 0 is (face N + j) N + i, level k >= 1 is 6 N N + face T + off_k + j N_k + i (T: the
// chain's texels of one face), which is its row in tex (6 N N, C) followed by mip (6 T, C).

struct CubeMipSizes : CubeSizes {
    int64_t T;        // texels of one face's packed chain (levels 1 .. nlev - 1); 6 (N N + T) < 2^31
    int nlev;
};

// one slot's sample: the taps of level j (a) and of level j + 1 (b), their idx the keys; f < 0: one level (b = a)
struct CubeMipTap {
    CubeTap a, b;
    float f;
    int j;
};

// cube_texel for a level of Nk x Nk faces whose face ``face`` starts at key base + face * fstride
__device__ __forceinline__ int cm_texel(int Nk, int fstride, int base, int face, int i, int j) {
    const bool ox = (unsigned)i >= (unsigned)Nk, oy = (unsigned)j >= (unsigned)Nk;
    if (ox || oy) {
        if (ox && oy) return -1;
        const int e = ox ? (i < 0 ? 0 : 1) : (j < 0 ? 2 : 3);
        const int k = ox ? j : i;
        const signed char* row = CUBE_SEAM[face][e];
        const int ne = row[1];
        const int kk = row[2] ? Nk - 1 - k : k;
        face = row[0];
        i = ne == 0 ? 0 : (ne == 1 ? Nk - 1 : kk);
        j = ne == 2 ? 0 : (ne == 3 ? Nk - 1 : kk);
    }
    return base + face * fstride + j * Nk + i;
}

// cube_tap's linear stage at level k of the chain: (sn, tn) are the face coordinates in [0, 1], computed once per slot
__device__ __forceinline__ CubeTap cm_level(const CubeMipSizes& z, int k, int face, float sn, float tn) {
    const int Nk = z.N >> k;
    int base = 0, fstride = z.N * z.N;
    if (k > 0) {
        base = (int)z.texels;                                                  // + off_k: the levels 1 .. k - 1 of one face
        for (int i = 1; i < k; i++) base += (z.N >> i) * (z.N >> i);
        fstride = (int)z.T;
    }
    const float x = sn * (float)Nk - 0.5f, y = tn * (float)Nk - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    CubeTap tap;
    tap.fx = x - x0; tap.fy = y - y0;
    const int i0 = min(max((int)x0, -1), Nk - 1), j0 = min(max((int)y0, -1), Nk - 1);
    const int t0 = cm_texel(Nk, fstride, base, face, i0, j0), t1 = cm_texel(Nk, fstride, base, face, i0 + 1, j0);
    const int t2 = cm_texel(Nk, fstride, base, face, i0, j0 + 1), t3 = cm_texel(Nk, fstride, base, face, i0 + 1, j0 + 1);
    tap.miss = t0 < 0 ? 0 : (t1 < 0 ? 1 : (t2 < 0 ? 2 : (t3 < 0 ? 3 : -1)));
    tap.idx[0] = t0 < 0 ? t3 : t0; tap.idx[1] = t1 < 0 ? t2 : t1; tap.idx[2] = t2 < 0 ? t1 : t2; tap.idx[3] = t3 < 0 ? t0 : t3;
    return tap;
}

// false = empty slot (nothing of ``tap`` or ``f`` is to be used)
__device__ __forceinline__ bool cm_tap(const CubeMipSizes& z, int64_t s, const int32_t* __restrict__ layers, const float* __restrict__ dirs,
                                       const float* __restrict__ level, CubeMipTap& tap, CubeFace& f) {
    if (!cube_face(z, s, layers, dirs, f)) return false;
    const float lod = level[s];
    if (!(fabsf(lod) < INFINITY)) return false;                                // NaN and infinities
    const float sn = 0.5f * (f.sc / f.ma + 1.0f), tn = 0.5f * (f.tc / f.ma + 1.0f);
    int j;
    if (lod <= 0.0f) { j = 0; tap.f = -1.0f; }
    else if (lod >= (float)(z.nlev - 1)) { j = z.nlev - 1; tap.f = -1.0f; }
    else { j = (int)floorf(lod); tap.f = lod - (float)j; }
    tap.j = j;
    tap.a = cm_level(z, j, f.face, sn, tn);
    tap.b = tap.a;
    if (tap.f >= 0.0f) tap.b = cm_level(z, j + 1, f.face, sn, tn);
    return true;
}

// the row of key ``key``: level 0 in tex, the rest in the chain (texv, mipv: the view's own where per view)
__device__ __forceinline__ const float* cm_row(const CubeMipSizes& z, const float* texv, const float* mipv, int key) {
    return key < (int)z.texels ? texv + (int64_t)key * z.C : mipv + ((int64_t)key - z.texels) * z.C;
}

// one level's sample of the V channels from c: k_texture_cube's linear sample through the key space
template <bool VEC4>
__device__ __forceinline__ TexQuad cm_sample(const CubeMipSizes& z, const float* texv, const float* mipv, int i00, int i10, int i01, int i11,
                                             int c, float fx, float fy, int miss) {
    const TexQuad t00 = tex_load_row<VEC4>(cm_row(z, texv, mipv, i00) + c), t10 = tex_load_row<VEC4>(cm_row(z, texv, mipv, i10) + c);
    const TexQuad t01 = tex_load_row<VEC4>(cm_row(z, texv, mipv, i01) + c), t11 = tex_load_row<VEC4>(cm_row(z, texv, mipv, i11) + c);
    if (miss < 0) return tex_blend_rows<VEC4>(t00, t10, t01, t11, fx, fy);
    const CornerW cw = cb_corner_w(fx, fy, miss);
    if (!VEC4) return {cb_corner(t00.x, t10.x, t01.x, t11.x, cw, miss), 0.0f, 0.0f, 0.0f};
    return {cb_corner(t00.x, t10.x, t01.x, t11.x, cw, miss), cb_corner(t00.y, t10.y, t01.y, t11.y, cw, miss),
            cb_corner(t00.z, t10.z, t01.z, t11.z, cw, miss), cb_corner(t00.w, t10.w, t01.w, t11.w, cw, miss)};
}

// VEC4: C is a multiple of 4 and tex / mip / out are 16-byte aligned; every channel goes through the same operations either way.
template <bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_cube_mip(CubeMipSizes z, const int32_t* __restrict__ layers, const float* __restrict__ dirs, const float* __restrict__ level,
                   const float* __restrict__ tex, const float* __restrict__ mip, float* __restrict__ out) {
    __shared__ int s_idx[8][TEX_BLOCK];                                        // s_idx[0] < 0: empty slot
    __shared__ float s_fx[2][TEX_BLOCK], s_fy[2][TEX_BLOCK], s_f[TEX_BLOCK];
    __shared__ int s_view[TEX_BLOCK];                                          // view * 64 + (miss_j + 1) * 8 + (miss_j+1 + 1)
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * TEX_BLOCK;
    const int nslots = (int)min((int64_t)TEX_BLOCK, z.S - s0);
    if (tid < nslots) {
        const int64_t s = s0 + tid;
        CubeMipTap tap;
        CubeFace f;
        const bool ok = cm_tap(z, s, layers, dirs, level, tap, f);
#pragma unroll
        for (int k = 0; k < 4; k++) { s_idx[k][tid] = ok ? tap.a.idx[k] : -1; s_idx[4 + k][tid] = ok ? tap.b.idx[k] : -1; }
        s_fx[0][tid] = ok ? tap.a.fx : 0.0f; s_fy[0][tid] = ok ? tap.a.fy : 0.0f;
        s_fx[1][tid] = ok ? tap.b.fx : 0.0f; s_fy[1][tid] = ok ? tap.b.fy : 0.0f;
        s_f[tid] = ok ? tap.f : -1.0f;
        s_view[tid] = (z.view_textures ? (int)(s / z.per_view) : 0) * 64 + (ok ? (tap.a.miss + 1) * 8 + (tap.b.miss + 1) : 0);
    }
    __syncthreads();
    constexpr int V = VEC4 ? 4 : 1;
    const int C = z.C, CV = C / V, total = nslots * CV;                      // lane -> (slot, group of V channels), group fastest
    const int dq = TEX_BLOCK / CV, dr = TEX_BLOCK - dq * CV;
    int slot = tid / CV, c = tid - slot * CV;
    float* o = out + s0 * C;
    for (int e = tid; e < total; e += TEX_BLOCK) {
        const int i00 = s_idx[0][slot];
        TexQuad r = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i00 >= 0) {
            const int vm = s_view[slot];
            const float* texv = tex + (int64_t)(vm >> 6) * z.texels * C;
            const float* mipv = mip + (int64_t)(vm >> 6) * 6 * z.T * C;
            const float f = s_f[slot];
            r = cm_sample<VEC4>(z, texv, mipv, i00, s_idx[1][slot], s_idx[2][slot], s_idx[3][slot], c * V, s_fx[0][slot], s_fy[0][slot],
                                ((vm >> 3) & 7) - 1);
            if (f >= 0.0f) {
                const TexQuad q = cm_sample<VEC4>(z, texv, mipv, s_idx[4][slot], s_idx[5][slot], s_idx[6][slot], s_idx[7][slot], c * V,
                                                  s_fx[1][slot], s_fy[1][slot], (vm & 7) - 1);
                r.x = r.x + f * (q.x - r.x);
                if (VEC4) { r.y = r.y + f * (q.y - r.y); r.z = r.z + f * (q.z - r.z); r.w = r.w + f * (q.w - r.w); }
            }
        }
        if (VEC4) reinterpret_cast<float4*>(o)[e] = make_float4(r.x, r.y, r.z, r.w);
        else o[e] = r.x;
        slot += dq; c += dr;
        if (c >= CV) { c -= CV; slot++; }
    }
}

// one level of one slot in the direction backward: the taps' rows, the fractions and what a corner needs; term() takes one
// channel, adds its part of (sum_c g d out / d fx, sum_c g d out / d fy) and returns the level's sample of that channel
struct CubeMipLevelDir {
    const float *p00, *p10, *p01, *p11;
    float fx, fy, su, sv;
    int miss;
    CornerW cw;
    CornerD d;
    __device__ __forceinline__ void init(const CubeMipSizes& z, const float* texv, const float* mipv, const CubeTap& t) {
        p00 = cm_row(z, texv, mipv, t.idx[0]); p10 = cm_row(z, texv, mipv, t.idx[1]);
        p01 = cm_row(z, texv, mipv, t.idx[2]); p11 = cm_row(z, texv, mipv, t.idx[3]);
        fx = t.fx; fy = t.fy; miss = t.miss; su = 0.0f; sv = 0.0f;
        cw = cb_corner_w(fx, fy, miss);
        const float gx = 1.0f - fx, gy = 1.0f - fy;
        d.x0 = miss == 0 ? 0.0f : -gy; d.x1 = miss == 1 ? 0.0f : gy; d.x2 = miss == 2 ? 0.0f : -fy; d.x3 = miss == 3 ? 0.0f : fy;
        d.y0 = miss == 0 ? 0.0f : -gx; d.y1 = miss == 1 ? 0.0f : -fx; d.y2 = miss == 2 ? 0.0f : gx; d.y3 = miss == 3 ? 0.0f : fx;
    }
    __device__ __forceinline__ float term(float t00, float t10, float t01, float t11, float g) {
        if (miss < 0) {
            tex_uv_term(t00, t10, t01, t11, g, fx, fy, su, sv);
            return tex_bilinear(t00, t10, t01, t11, fx, fy);
        }
        cb_dir_term_corner(t00, t10, t01, t11, g, cw, d, miss, su, sv);
        return cb_corner(t00, t10, t01, t11, cw, miss);
    }
    // the sums in texel units of the level (a corner's 1 / W applied to the sums, as in k_texture_cube_bwd_dir)
    __device__ __forceinline__ void finish() { if (miss >= 0) { su = su / cw.W; sv = sv / cw.W; } }
};

// VEC4 as in k_texture_cube_bwd_dir: the sums run over the channels in the same order either way.  dL_dout4: (B,H,W,L,4) rows
// (dL/ddir.x, .y, .z, dL/dlod).
template <bool VEC4>
__global__ void __launch_bounds__(TEX_BLOCK)
k_texture_cube_mip_bwd_dir(CubeMipSizes z, const int32_t* __restrict__ layers, const float* __restrict__ dirs,
                           const float* __restrict__ level, const float* __restrict__ tex, const float* __restrict__ mip,
                           const float* __restrict__ g, float* __restrict__ dL_dout4) {
    const int64_t s = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
    if (s >= z.S) return;
    CubeMipTap tap;
    CubeFace f;
    float dx = 0.0f, dy = 0.0f, dz = 0.0f, dl = 0.0f;
    if (cm_tap(z, s, layers, dirs, level, tap, f)) {
        const int C = z.C;
        const int64_t view = z.view_textures ? s / z.per_view : 0;
        const float* texv = tex + view * z.texels * C;
        const float* mipv = mip + view * 6 * z.T * C;
        const float* gs = g + s * C;
        const bool two = tap.f >= 0.0f;
        CubeMipLevelDir a, b;
        a.init(z, texv, mipv, tap.a);
        b.init(z, texv, mipv, tap.b);
        if (two) {
            if (VEC4) {
                for (int c = 0; c < C; c += 4) {
                    const float4 a00 = *reinterpret_cast<const float4*>(a.p00 + c), a10 = *reinterpret_cast<const float4*>(a.p10 + c);
                    const float4 a01 = *reinterpret_cast<const float4*>(a.p01 + c), a11 = *reinterpret_cast<const float4*>(a.p11 + c);
                    const float4 b00 = *reinterpret_cast<const float4*>(b.p00 + c), b10 = *reinterpret_cast<const float4*>(b.p10 + c);
                    const float4 b01 = *reinterpret_cast<const float4*>(b.p01 + c), b11 = *reinterpret_cast<const float4*>(b.p11 + c);
                    const float4 gv = *reinterpret_cast<const float4*>(gs + c);
                    dl += gv.x * (b.term(b00.x, b10.x, b01.x, b11.x, gv.x) - a.term(a00.x, a10.x, a01.x, a11.x, gv.x));
                    dl += gv.y * (b.term(b00.y, b10.y, b01.y, b11.y, gv.y) - a.term(a00.y, a10.y, a01.y, a11.y, gv.y));
                    dl += gv.z * (b.term(b00.z, b10.z, b01.z, b11.z, gv.z) - a.term(a00.z, a10.z, a01.z, a11.z, gv.z));
                    dl += gv.w * (b.term(b00.w, b10.w, b01.w, b11.w, gv.w) - a.term(a00.w, a10.w, a01.w, a11.w, gv.w));
                }
            } else {
                for (int c = 0; c < C; c++) {
                    const float gc = gs[c];
                    dl += gc * (b.term(b.p00[c], b.p10[c], b.p01[c], b.p11[c], gc) - a.term(a.p00[c], a.p10[c], a.p01[c], a.p11[c], gc));
                }
            }
        } else {
            if (VEC4) {
                for (int c = 0; c < C; c += 4) {
                    const float4 a00 = *reinterpret_cast<const float4*>(a.p00 + c), a10 = *reinterpret_cast<const float4*>(a.p10 + c);
                    const float4 a01 = *reinterpret_cast<const float4*>(a.p01 + c), a11 = *reinterpret_cast<const float4*>(a.p11 + c);
                    const float4 gv = *reinterpret_cast<const float4*>(gs + c);
                    a.term(a00.x, a10.x, a01.x, a11.x, gv.x); a.term(a00.y, a10.y, a01.y, a11.y, gv.y);
                    a.term(a00.z, a10.z, a01.z, a11.z, gv.z); a.term(a00.w, a10.w, a01.w, a11.w, gv.w);
                }
            } else {
                for (int c = 0; c < C; c++) a.term(a.p00[c], a.p10[c], a.p01[c], a.p11[c], gs[c]);
            }
        }
        a.finish();
        // x_k = s N_k - 0.5, s = 0.5 (u + 1), u = sc / ma: each level's sums with its own N_k, blended by (1 - f, f)
        const float Nj = (float)(z.N >> tap.j);
        float A = 0.5f * Nj * a.su, Bq = 0.5f * Nj * a.sv;
        if (two) {
            b.finish();
            const float N1 = (float)(z.N >> (tap.j + 1));
            A = (1.0f - tap.f) * A + tap.f * (0.5f * N1 * b.su);
            Bq = (1.0f - tap.f) * Bq + tap.f * (0.5f * N1 * b.sv);
        }
        const float inv = 1.0f / f.ma;
        const float dsc = A * inv, dtc = Bq * inv, dma = -((A * f.sc + Bq * f.tc) * inv) * inv;
        const int neg = f.face & 1;
        const float dmaj = neg ? -dma : dma;
        if (f.face < 2) { dx = dmaj; dy = -dtc; dz = neg ? dsc : -dsc; }
        else if (f.face < 4) { dx = dsc; dy = dmaj; dz = neg ? -dtc : dtc; }
        else { dx = neg ? -dsc : dsc; dy = -dtc; dz = dmaj; }
    }
    reinterpret_cast<float4*>(dL_dout4)[s] = make_float4(dx, dy, dz, dl);
}

template <int CH>
__global__ void __launch_bounds__(TILE_PIX)
k_texture_cube_mip_bwd_tex(CubeMipSizes z, const int32_t* __restrict__ layers, const float* __restrict__ dirs,
                           const float* __restrict__ level, const float* __restrict__ g, float* __restrict__ dL_dtex,
                           float* __restrict__ dL_dmip) {
    __shared__ TexTable<CH> tab;
    const int b = blockIdx.z, tid = threadIdx.x;
    const TilePixel t = tile_pixel(tid, z.W, z.H);
    const int C = z.C, L = z.L;
    const int texels = (int)z.texels;
    // either may be null (not wanted): its texels are skipped
    float* dtex = dL_dtex ? dL_dtex + (z.view_textures ? (int64_t)b * z.texels * C : 0) : nullptr;
    float* dmip = dL_dmip ? dL_dmip + (z.view_textures ? (int64_t)b * 6 * z.T * C : 0) : nullptr;
    auto row = [&](int key) -> float* {
        if (key < texels) return dtex ? dtex + (int64_t)key * C : nullptr;
        return dmip ? dmip + (int64_t)(key - texels) * C : nullptr;
    };
    // the coarse levels whose cubes together take at most half the table: their keys claim their slots first (tex_scatter_layer_masked)
    int k_hot = z.nlev;
    for (int m = z.nlev - 1, acc = 0; m >= 0; m--) {
        acc += 6 * (z.N >> m) * (z.N >> m);
        if (acc > LC_SLOTS / 2) break;
        k_hot = m;
    }
    for (int l = 0; l < L; l++) {
        const int64_t s = t.pix * L + l;
        CubeMipTap tap = {{{0, 0, 0, 0}, 0.0f, 0.0f, -1}, {{0, 0, 0, 0}, 0.0f, 0.0f, -1}, -1.0f, 0};
        CubeFace f;
        const bool live = t.inside && cm_tap(z, s, layers, dirs, level, tap, f);
        const bool two = tap.f >= 0.0f;
        const float wl[2] = {two ? 1.0f - tap.f : 1.0f, two ? tap.f : 0.0f};
        // (the eight pairs as flat lists, level j's four first)
        const int key[8] = {tap.a.idx[0], tap.a.idx[1], tap.a.idx[2], tap.a.idx[3], tap.b.idx[0], tap.b.idx[1], tap.b.idx[2], tap.b.idx[3]};
        float w[8];
        unsigned mask = two ? 0xFFu : 0x0Fu;                                   // pair 4 lv + k takes part
#pragma unroll
        for (int lv = 0; lv < 2; lv++) {
            const CubeTap& q = lv ? tap.b : tap.a;
            const float fx = q.fx, fy = q.fy;
            float w0 = (1.0f - fx) * (1.0f - fy), w1 = fx * (1.0f - fy), w2 = (1.0f - fx) * fy, w3 = fx * fy;
            if (q.miss >= 0) {                                                 // a corner: the three weights over their sum, no fourth
                const CornerW cw = cb_corner_w(fx, fy, q.miss);
                w0 = cw.w0 / cw.W; w1 = cw.w1 / cw.W; w2 = cw.w2 / cw.W; w3 = cw.w3 / cw.W;
                mask &= ~(1u << (4 * lv + q.miss));
            }
            w[4 * lv] = wl[lv] * w0; w[4 * lv + 1] = wl[lv] * w1; w[4 * lv + 2] = wl[lv] * w2; w[4 * lv + 3] = wl[lv] * w3;
        }
        const unsigned first = (tap.j >= k_hot ? 0x0Fu : 0u) | (tap.j + 1 >= k_hot ? 0xF0u : 0u);
        tex_scatter_layer_masked<CH, 8, true>(tab, tid, live, key, w, mask, first, g, s, C, row);
    }
}

static CubeMipSizes cm_sizes(int B, int H, int W, int L, int N, int C, int view_textures, int max_level) {
    CubeMipSizes z;
    tex_common_sizes(z, B, H, W, L, C, view_textures);
    z.texels = (int64_t)6 * N * N;
    z.N = N;
    z.nlev = mip_levels(N, N, max_level, &z.T);
    return z;
}

void launch_texture_cube_mip(int B, int H, int W, int L, int N, int C, int view_textures, int max_level, const int32_t* render_layers,
                             const float* dirs, const float* level, const float* tex, const float* mip, float* out, hipStream_t st) {
    const CubeMipSizes z = cm_sizes(B, H, W, L, N, C, view_textures, max_level);
    const dim3 grid = tex_flat_grid(z.S);
    if (C % 4 == 0 && tex_aligned16(tex, out, mip))
        hipLaunchKernelGGL((k_texture_cube_mip<true>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, dirs, level, tex, mip, out);
    else
        hipLaunchKernelGGL((k_texture_cube_mip<false>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, dirs, level, tex, mip, out);
}

void launch_texture_cube_mip_backward(int B, int H, int W, int L, int N, int C, int view_textures, int max_level,
                                      const int32_t* render_layers, const float* dirs, const float* level, const float* tex,
                                      const float* mip, const float* dL_dout, float* dL_dtex, float* dL_dmip, float* dL_ddir_level,
                                      hipStream_t st) {
    const CubeMipSizes z = cm_sizes(B, H, W, L, N, C, view_textures, max_level);
    if (dL_ddir_level) {
        const dim3 grid = tex_flat_grid(z.S);
        if (C % 4 == 0 && tex_aligned16(tex, mip, dL_dout))
            hipLaunchKernelGGL((k_texture_cube_mip_bwd_dir<true>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, dirs, level, tex, mip,
                               dL_dout, dL_ddir_level);
        else
            hipLaunchKernelGGL((k_texture_cube_mip_bwd_dir<false>), grid, dim3(TEX_BLOCK), 0, st, z, render_layers, dirs, level, tex, mip,
                               dL_dout, dL_ddir_level);
    }
    if (dL_dtex || dL_dmip) {
        const dim3 grid = tile_grid(W, H, B);
#define DM2_CM_TEX(CH) hipLaunchKernelGGL((k_texture_cube_mip_bwd_tex<CH>), grid, dim3(TILE_PIX), 0, st, z, render_layers, dirs, level, dL_dout, dL_dtex, dL_dmip)
        if (C == 1) DM2_CM_TEX(1); else if (C == 2) DM2_CM_TEX(2); else if (C == 3) DM2_CM_TEX(3); else DM2_CM_TEX(TEX_CH);
#undef DM2_CM_TEX
    }
}

}  // namespace dm2
