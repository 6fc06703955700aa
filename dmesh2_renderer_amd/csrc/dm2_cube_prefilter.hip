// dm2_cube_prefilter.hip -- Renderer.cube_prefilter: the GGX prefilter of a cube's mip chain and its transpose.
//
// Contract: include/dm2_hip.h, dm2_cube_prefilter.  Level k of the chain (faces of n = N >> k) is
// filtered from the same level of the input with the lobe K(o,s) of roughness k / (nlev - 1):
//   forward:   y[o,c]    = sum_s (K(o,s) Om_s) x[s,c]
//   transpose: xbar[s,c] = Om_s sum_o K(o,s) ybar[o,c]
// K is symmetric to the bit, so one kernel serves both: a thread owns one texel and gathers over all the others; the solid
// angle Om multiplies each term (forward: the gathered texel's) or the finished sum (transpose: the thread's own).
//
// A block owns a 16 x 16 tile of one face and a chunk of CH channels.  It walks the tiles of all six faces: 256 at a time, each
// thread tests one tile's bounding ball against the block's (pf_ball; a ballot per wave leaves the verdicts in LDS, so the walk
// is in tile order: a pure function of the inputs), and every tile that can hold a member is staged through LDS as rows of
// (d, Om) plus the chunk's values, computed while staging.  In the pair loop every lane reads the same row: a broadcast.
// A level with small faces (up to 64^2) would leave most of the device idle that way, with a few blocks each walking every
// texel: there a block owns 4 x 4 outputs, 16 threads share each output's walk (thread p takes rows p, p + 16, ... of a staged
// tile) and their sums are added in the order of p through LDS.  Either way the order is fixed: two calls give the same bits.
//
// The tile test is conservative: for texels o, s of tiles with ball centres A_o, A_s and radii rho_o, rho_s (in chord length),
// |d_o - d_s| >= |A_o - A_s| - rho_o - rho_s, and a member has |d_o - d_s|^2 = m <= min(2, 252 a2 / (1 - a2)) (c > 0 and
// e <= 64 a2 in real numbers); the test allows 1e-3 of chord on top, orders of magnitude above the fp32 rounding of either
// side.  rho is the largest distance from A to a corner texel of the tile: d . A = (p . A) / |p| is quasi-concave in the face's
// plane where it is not negative, so over the rectangle of texel centres its minimum lies at a corner (a tile one of whose
// corners has d . A < 0 gets rho = 2 and is never skipped; on a cube's face none has).
#include <hip/hip_runtime.h>

#include <cmath>

#include "dm2_state.h"

namespace dm2 {
namespace {

constexpr int PF_TILE = 16;
constexpr int PF_BLOCK = PF_TILE * PF_TILE;
constexpr int PF_MAX_CH = 4;
constexpr int PF_SPLIT_FACE = 64;      // faces up to this size: output tiles of PF_SPLIT_TILE^2, 16 threads per output
constexpr int PF_SPLIT_TILE = 4;

struct PfLevel {
    int n;               // the level's face extent
    int tiles;           // tiles along a face's side
    int C;
    int64_t T;           // texels of one face's chain
    int64_t off;         // the level's first texel in a face's chain
    float a2, one_minus_a2, cut;      // cut = 64 a2
    float reach;         // sqrt(the largest m a member can have) + 1e-3
};

// (d.x, d.y, d.z, Om) of texel (face, j, i): the contract's formulas in the written order
__device__ __forceinline__ float4 pf_texel(int face, int i, int j, float fn) {
    const float sc = (2.0f * ((float)i + 0.5f)) / fn - 1.0f;
    const float tc = (2.0f * ((float)j + 0.5f)) / fn - 1.0f;
    const float q = (1.0f + sc * sc) + tc * tc;
    const float rq = sqrtf(q);
    float px, py, pz;                                                    // the inverse of the lookup's table
    switch (face) {
        case 0: px = 1.0f; py = -tc; pz = -sc; break;                   // +x: sc = -z, tc = -y
        case 1: px = -1.0f; py = -tc; pz = sc; break;                   // -x: sc = +z, tc = -y
        case 2: px = sc; py = 1.0f; pz = tc; break;                     // +y: sc = +x, tc = +z
        case 3: px = sc; py = -1.0f; pz = -tc; break;                   // -y: sc = +x, tc = -z
        case 4: px = sc; py = -tc; pz = 1.0f; break;                    // +z: sc = +x, tc = -y
        default: px = -sc; py = -tc; pz = -1.0f; break;                 // -z: sc = -x, tc = -y
    }
    return make_float4(px / rq, py / rq, pz / rq, 1.0f / (q * rq));
}

// the bounding ball of the texels [i0, i0 + side) x [j0, j0 + side) of ``face``, clipped to the face: (centre A on the sphere,
// rho = the largest chord from A to one of them)
__device__ __forceinline__ float4 pf_ball(int face, int i0, int j0, int side, int n, float fn) {
    const int i1 = min(i0 + side, n) - 1, j1 = min(j0 + side, n) - 1;
    const float4 c[4] = {pf_texel(face, i0, j0, fn), pf_texel(face, i1, j0, fn), pf_texel(face, i0, j1, fn), pf_texel(face, i1, j1, fn)};
    float ax = (c[0].x + c[1].x) + (c[2].x + c[3].x), ay = (c[0].y + c[1].y) + (c[2].y + c[3].y), az = (c[0].z + c[1].z) + (c[2].z + c[3].z);
    const float len = sqrtf((ax * ax + ay * ay) + az * az);
    ax = ax / len; ay = ay / len; az = az / len;
    float rho2 = 0.0f, low = 1.0f;
    for (int k = 0; k < 4; k++) {
        const float dx = c[k].x - ax, dy = c[k].y - ay, dz = c[k].z - az;
        rho2 = fmaxf(rho2, (dx * dx + dy * dy) + dz * dz);
        low = fminf(low, (c[k].x * ax + c[k].y * ay) + c[k].z * az);
    }
    return make_float4(ax, ay, az, low >= 0.0f ? sqrtf(rho2) : 2.0f);    // (a NaN centre fails the comparison: never skipped)
}

template <int CH, int OT, bool TRANSPOSE>
__global__ void __launch_bounds__(PF_BLOCK)
k_cube_prefilter(PfLevel z, const float* __restrict__ x, float* __restrict__ y) {
    __shared__ float4 s_geo[PF_BLOCK];
    __shared__ __align__(16) float s_val[PF_BLOCK * CH];
    __shared__ unsigned long long s_reach[PF_BLOCK / 64];
    constexpr int OUTS = OT * OT, PARTS = PF_BLOCK / OUTS;               // thread -> (output texel, share of each staged tile)
    __shared__ float s_sum[PARTS > 1 ? PF_BLOCK * CH : 1];

    const int tid = threadIdx.x;
    const int tpf = z.tiles * z.tiles, ntiles = 6 * tpf;
    const int otiles = (z.n + OT - 1) / OT, otpf = otiles * otiles;
    const int oface = (int)blockIdx.x / otpf, ot = (int)blockIdx.x - oface * otpf;
    const int oty = ot / otiles, otx = ot - oty * otiles;
    const int o = tid & (OUTS - 1), part = tid / OUTS;
    const int c0 = (int)blockIdx.y * CH;
    const int64_t face_stride = z.T * z.C;                               // floats of one face's chain
    const float* xc = x + (int64_t)blockIdx.z * 6 * face_stride;
    float* yc = y + (int64_t)blockIdx.z * 6 * face_stride;
    const float fn = (float)z.n;

    const int oi = otx * OT + (o & (OT - 1)), oj = oty * OT + o / OT;
    const bool live = oi < z.n && oj < z.n;
    const float4 od = pf_texel(oface, min(oi, z.n - 1), min(oj, z.n - 1), fn);
    const float4 ob = pf_ball(oface, otx * OT, oty * OT, OT, z.n, fn);

    float acc[CH];
#pragma unroll
    for (int ch = 0; ch < CH; ch++) acc[ch] = 0.0f;

    for (int base = 0; base < ntiles; base += PF_BLOCK) {
        // one tile per thread: can it hold a member of any texel of this block's tile?
        bool reach = false;
        const int cand = base + tid;
        if (cand < ntiles) {
            const int f = cand / tpf, t = cand - f * tpf;
            const int ty = t / z.tiles, tx = t - ty * z.tiles;
            const float4 sb = pf_ball(f, tx * PF_TILE, ty * PF_TILE, PF_TILE, z.n, fn);
            const float dx = ob.x - sb.x, dy = ob.y - sb.y, dz = ob.z - sb.z;
            const float gap = (sqrtf((dx * dx + dy * dy) + dz * dz) - ob.w) - sb.w;
            reach = !(gap > z.reach);
        }
        const unsigned long long verdicts = __ballot(reach);
        __syncthreads();                                                 // (the last batch's verdicts and rows are read)
        if ((tid & 63) == 0) s_reach[tid >> 6] = verdicts;
        __syncthreads();
        unsigned long long bits[PF_BLOCK / 64];
#pragma unroll
        for (int w = 0; w < PF_BLOCK / 64; w++) bits[w] = s_reach[w];

#pragma unroll
        for (int w = 0; w < PF_BLOCK / 64; w++) {
            while (bits[w]) {                                            // (uniform over the block: every thread read the same words)
                const int stile = base + w * 64 + (__ffsll((long long)bits[w]) - 1);
                bits[w] &= bits[w] - 1;
                const int sface = stile / tpf, st = stile - sface * tpf;
                const int sty = st / z.tiles, stx = st - sty * z.tiles;
                const int tw = min(PF_TILE, z.n - stx * PF_TILE), th = min(PF_TILE, z.n - sty * PF_TILE);
                const int cnt = tw * th;                                 // the tile's texels, packed: row jj * tw + ii
                __syncthreads();                                         // (the rows of the tile before are read)
                if (tid < cnt) {
                    const int jj = tid / tw, ii = tid - jj * tw;
                    const int si = stx * PF_TILE + ii, sj = sty * PF_TILE + jj;
                    s_geo[tid] = pf_texel(sface, si, sj, fn);
                    const float* row = xc + (int64_t)sface * face_stride + (z.off + (int64_t)sj * z.n + si) * z.C;
#pragma unroll
                    for (int ch = 0; ch < CH; ch++) s_val[tid * CH + ch] = c0 + ch < z.C ? row[c0 + ch] : 0.0f;
                }
                __syncthreads();
#pragma unroll 4
                for (int s = part; s < cnt; s += PARTS) {
                    const float4 g = s_geo[s];
                    const float dx = od.x - g.x, dy = od.y - g.y, dz = od.z - g.z;
                    const float m = (dx * dx + dy * dy) + dz * dz;
                    const float c = 1.0f - 0.5f * m;
                    const float e = z.a2 + z.one_minus_a2 * (0.25f * m);
                    const float t = z.a2 / e;
                    const float k = (t * t) * c;
                    const bool member = c > 0.0f && e <= z.cut;
                    const float wgt = member ? (TRANSPOSE ? k : k * g.w) : 0.0f;
#pragma unroll
                    for (int ch = 0; ch < CH; ch++) acc[ch] = acc[ch] + wgt * s_val[s * CH + ch];
                }
            }
        }
    }

    if (PARTS > 1) {                                                     // the shares of one output, summed in their order
#pragma unroll
        for (int ch = 0; ch < CH; ch++) s_sum[tid * CH + ch] = acc[ch];
        __syncthreads();
        if (part == 0) {
#pragma unroll
            for (int ch = 0; ch < CH; ch++) {
                float sum = acc[ch];
                for (int p = 1; p < PARTS; p++) sum = sum + s_sum[(p * OUTS + o) * CH + ch];
                acc[ch] = sum;
            }
        }
    }
    if (live && part == 0) {
        float* row = yc + (int64_t)oface * face_stride + (z.off + (int64_t)oj * z.n + oi) * z.C;
#pragma unroll
        for (int ch = 0; ch < CH; ch++)
            if (c0 + ch < z.C) row[c0 + ch] = TRANSPOSE ? od.w * acc[ch] : acc[ch];
    }
}

template <int CH>
void pf_launch(const PfLevel& z, int cubes, int transpose, const float* x, float* y, hipStream_t st) {
    // faces up to PF_SPLIT_FACE: 16 times the blocks, each output's sum shared by 16 threads (a level of 16^2 faces has 6 tiles)
    const int ot = z.n <= PF_SPLIT_FACE ? PF_SPLIT_TILE : PF_TILE;
    const int otiles = (z.n + ot - 1) / ot;
    const dim3 grid(6 * otiles * otiles, (z.C + CH - 1) / CH, cubes);
#define DM2_PF(OT, TR) hipLaunchKernelGGL((k_cube_prefilter<CH, OT, TR>), grid, dim3(PF_BLOCK), 0, st, z, x, y)
    if (ot == PF_TILE) { if (transpose) DM2_PF(PF_TILE, true); else DM2_PF(PF_TILE, false); }
    else { if (transpose) DM2_PF(PF_SPLIT_TILE, true); else DM2_PF(PF_SPLIT_TILE, false); }
#undef DM2_PF
}

}  // namespace

int cube_prefilter_max_channels() { return PF_MAX_CH * 65535; }

void launch_cube_prefilter(int cubes, int N, int C, int max_level, int transpose, const float* x, float* y, hipStream_t st) {
    int64_t T;
    const int nlev = mip_levels(N, N, max_level, &T);
    int64_t off = 0;
    for (int k = 1; k < nlev; k++) {
        PfLevel z;
        z.n = N >> k;
        z.tiles = (z.n + PF_TILE - 1) / PF_TILE;
        z.C = C; z.T = T; z.off = off;
        const float r = (float)k / (float)(nlev - 1);
        const float a = r * r;
        z.a2 = a * a;
        z.one_minus_a2 = 1.0f - z.a2;
        z.cut = 64.0f * z.a2;
        double mmax = 2.0;                                               // c > 0
        if (z.a2 < 1.0f) mmax = std::fmin(mmax, 252.0 * (double)z.a2 / (1.0 - (double)z.a2));      // e <= 64 a2
        z.reach = (float)(std::sqrt(mmax) + 1e-3);
        switch (C < PF_MAX_CH ? C : PF_MAX_CH) {
            case 1: pf_launch<1>(z, cubes, transpose, x, y, st); break;
            case 2: pf_launch<2>(z, cubes, transpose, x, y, st); break;
            case 3: pf_launch<3>(z, cubes, transpose, x, y, st); break;
            default: pf_launch<4>(z, cubes, transpose, x, y, st); break;
        }
        off += (int64_t)z.n * z.n;
    }
}

}  // namespace dm2
