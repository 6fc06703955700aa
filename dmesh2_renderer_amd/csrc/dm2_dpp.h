// dm2_dpp.h -- DPP row-shift helpers and the segmented scans used by the backward kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace dm2 {

// DPP row shifts (16-lane rows; lanes shifted in from outside the row read 0)
template <int N> __device__ __forceinline__ int dpp_shr_i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x110 + N, 0xF, 0xF, true); }
template <int N> __device__ __forceinline__ int dpp_shl_i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x100 + N, 0xF, 0xF, true); }
template <int N> __device__ __forceinline__ float dpp_shr_f(float v) { return __int_as_float(dpp_shr_i<N>(__float_as_int(v))); }
// inclusive segmented sum inside a row of 16 lanes; sK = "lane l-K belongs to the same run"
// (written as "add the shifted value, then keep the sum where the lane continues a run" so that the compiler can fold
// the DPP move into the add: v_add_f32_dpp + v_cndmask per step instead of v_mov_dpp + v_cndmask + v_add)
__device__ __forceinline__ void seg_scan16(float& v, bool s1, bool s2, bool s4, bool s8) {
    float t = v + dpp_shr_f<1>(v); v = s1 ? t : v;
    t = v + dpp_shr_f<2>(v); v = s2 ? t : v;
    t = v + dpp_shr_f<4>(v); v = s4 ? t : v;
    t = v + dpp_shr_f<8>(v); v = s8 ? t : v;
}

// The same segmented scan for N values at once with ONE instruction per value and step: v_fmac_f32 with a DPP source,
//     v += shifted(v) * mK,      mK = 1.0 where lane l - K continues the lane's run, else 0.0
// (t * 1.0 + v rounds once, exactly like t + v; lanes shifted in from outside the row read 0).  Inline assembly: the
// compiler has no pattern that folds a select into a DPP multiply-add.  A DPP read needs two wait states behind the VALU
// write of its source; the steps of one value are N >= 3 instructions apart, and an s_nop covers the producers.
// Requires finite values (0 * inf would poison a lane that is not part of the run).
template <int N>
__device__ __forceinline__ void seg_scan16_n(float (&g)[N], float m1, float m2, float m4, float m8) {
    static_assert(N >= 3, "the steps of one value must be at least three instructions apart");
    asm volatile("s_nop 1");
#pragma unroll
    for (int c = 0; c < N; c++) asm volatile("v_fmac_f32_dpp %0, %0, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(g[c]) : "v"(m1));
#pragma unroll
    for (int c = 0; c < N; c++) asm volatile("v_fmac_f32_dpp %0, %0, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(g[c]) : "v"(m2));
#pragma unroll
    for (int c = 0; c < N; c++) asm volatile("v_fmac_f32_dpp %0, %0, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(g[c]) : "v"(m4));
#pragma unroll
    for (int c = 0; c < N; c++) asm volatile("v_fmac_f32_dpp %0, %0, %1 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(g[c]) : "v"(m8));
}

// seg_scan16_n for values that may not be finite (a sliver face whose determinant underflows, a NaN vertex): the
// multiply-by-0 continuation mask of the fast form would turn a neighbouring run's Inf into NaN in THIS run, so a wave in
// which any lane holds a non-finite value takes the select form (two instructions per value and step), which keeps a
// non-finite gradient inside the rows of the face that produced it, as the reference's per-pair atomics do.
template <int N>
__device__ __forceinline__ void seg_scan16_safe(float (&g)[N], float m1, float m2, float m4, float m8, bool s1, bool s2, bool s4, bool s8) {
    float mag = 0.f;
#pragma unroll
    for (int c = 0; c < N; c++) mag += fabsf(g[c]);
    if (__builtin_expect(__ballot(!(mag < 3.0e38f)) == 0ull, 1)) { seg_scan16_n(g, m1, m2, m4, m8); return; }
#pragma unroll
    for (int c = 0; c < N; c++) seg_scan16(g[c], s1, s2, s4, s8);
}

// ---- runs anywhere in the wave: the row scan plus two cross-row steps, one total per run and wave -------------------------
// Everything is derived from ONE wave-uniform word, the ballot `cont` of "lane l continues lane l - 1, the same run" (bit 0
// clear), with scalar operations at the point of use -- a run is a stretch of lanes, so "lane l - K is in my run" is "the K
// lanes up to l all continue".  The words live in scalar registers, where per-lane predicates or multipliers would each hold
// a vector register across the caller's phase (the backward's kernels have none to spare).  A caller that clears the bits
// of the rows' first lanes (16, 32, 48) in `cont` gets runs that end at the rows, and no cross-row step.
//   b1, b2, b4, b8  row_shr:K      lane l takes the step: lane l - K is in its row and in its run
//   b15             row_bcast:15   rows 1 and 3: the lane's run reaches back to its row's first lane AND on into the row before
//                                  (every lane from the row's first up to l continues its predecessor)
//   b31             row_bcast:31   rows 2 and 3: every lane from 32 up to l does
// Behind the four row steps a lane holds the sum of its run from the run's start (or its row's) up to itself; lane 15 / 47
// then carries its part into the lanes of the next row that continue it, then lane 31 (complete by then) into rows 2 and 3.
struct SegSteps { unsigned long long b1, b2, b4, b8, b15, b31; };
__device__ __forceinline__ SegSteps seg_steps(unsigned long long cont) {
    SegSteps k;
    k.b1 = cont & ~0x0001000100010001ull;                                        // (a row's first lane has no lane l - 1 in its row)
    k.b2 = k.b1 & (k.b1 << 1);
    k.b4 = k.b2 & (k.b2 << 2);
    k.b8 = k.b4 & (k.b4 << 4);
    const unsigned long long stop = ~cont;                                       // run starts
    // the lanes below a row's (a half's) first run start: lowest set bit - 1; all of them where there is none
    const uint32_t t1 = (uint32_t)(stop >> 16) & 0xFFFFu, t3 = (uint32_t)(stop >> 48), th = (uint32_t)(stop >> 32);
    const uint32_t r1 = ((t1 & (0u - t1)) - 1u) & 0xFFFFu, r3 = ((t3 & (0u - t3)) - 1u) & 0xFFFFu;
    k.b15 = ((unsigned long long)r1 << 16) | ((unsigned long long)r3 << 48);
    k.b31 = (unsigned long long)((th & (0u - th)) - 1u) << 32;
    return k;
}
__device__ __forceinline__ bool lane_bit(unsigned long long b, int lane) {
    return (((lane & 32) ? (uint32_t)(b >> 32) : (uint32_t)b) >> (lane & 31) & 1u) != 0u;
}
// the lane of a run that holds the run's total behind all six steps: lane l + 1 does not continue it (lane 63: nothing does)
__device__ __forceinline__ bool run_last_lane(unsigned long long cont, int lane) { return !lane_bit(cont >> 1, lane); }

__device__ __forceinline__ float dpp_bcast15_f(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xA, 0xF, false)); }
__device__ __forceinline__ float dpp_bcast31_f(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xC, 0xF, false)); }
// select form, one value (seg_scan16 and the two cross-row steps); non-finite values stay in their run
__device__ __forceinline__ void seg_scan64(float& v, unsigned long long cont, int lane) {
    const SegSteps k = seg_steps(cont);
    seg_scan16(v, lane_bit(k.b1, lane), lane_bit(k.b2, lane), lane_bit(k.b4, lane), lane_bit(k.b8, lane));
    const bool c15 = lane_bit(k.b15, lane), c31 = lane_bit(k.b31, lane);
    float t = v + dpp_bcast15_f(v); v = c15 ? t : v;
    t = v + dpp_bcast31_f(v); v = c31 ? t : v;
}

// All six steps for N values at once with ONE instruction per value and step: v_fmac_f32 with a DPP source,
//     v += read(v) * m,      m = 1.0 where the lane takes the step, else 0.0
// (t * 1.0 + v rounds once, exactly like t + v; lanes shifted in from outside the row read 0).  Inline assembly: the
// compiler has no pattern that folds a select into a DPP multiply-add.  The multiplier of a step is made from the step's
// ballot right in front of the step and dies behind it.  A DPP read needs two wait states behind the VALU write of its
// source: the select and the N - 1 other values (N >= 3) stand between a value's write and its next DPP read, and an s_nop
// covers the producers.  Requires finite values (0 * inf would poison a lane that is not part of the run).
#define DM2_SEG_STEP(CTRL, BAL)                                                                                            \
    asm volatile("v_cndmask_b32_e64 %0, 0, 1.0, %1" : "=v"(m) : "s"(BAL));                                                 \
    _Pragma("unroll") for (int c = 0; c < N; c++)                                                                          \
        asm volatile("v_fmac_f32_dpp %0, %0, %1 " CTRL : "+v"(g[c]) : "v"(m));
template <int N>
__device__ __forceinline__ void seg_scan64_n(float (&g)[N], const SegSteps& k) {
    static_assert(N >= 3, "the steps of one value must be at least three instructions apart");
    float m;
    asm volatile("s_nop 1");
    DM2_SEG_STEP("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1", k.b1)
    DM2_SEG_STEP("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1", k.b2)
    DM2_SEG_STEP("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1", k.b4)
    DM2_SEG_STEP("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1", k.b8)
    if ((k.b15 | k.b31) == 0ull) return;                                          // (wave-uniform: no run of this wave crosses a row)
    DM2_SEG_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf", k.b15)
    DM2_SEG_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf", k.b31)
}
#undef DM2_SEG_STEP
// the same for one finite value (a count): the next step's select and one s_nop stand in for the other values
__device__ __forceinline__ void seg_scan64_finite(float& v, const SegSteps& k) {
    float m;
#define DM2_SEG_STEP1(CTRL, BAL)                                                                                           \
    asm volatile("v_cndmask_b32_e64 %0, 0, 1.0, %2\n s_nop 0\n v_fmac_f32_dpp %1, %1, %0 " CTRL : "=&v"(m), "+v"(v) : "s"(BAL));
    asm volatile("s_nop 1");
    DM2_SEG_STEP1("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1", k.b1)
    DM2_SEG_STEP1("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1", k.b2)
    DM2_SEG_STEP1("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1", k.b4)
    DM2_SEG_STEP1("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1", k.b8)
    if ((k.b15 | k.b31) != 0ull) {
        DM2_SEG_STEP1("row_bcast:15 row_mask:0xa bank_mask:0xf", k.b15)
        DM2_SEG_STEP1("row_bcast:31 row_mask:0xc bank_mask:0xf", k.b31)
    }
#undef DM2_SEG_STEP1
}

// Inclusive segmented sum of N values over the runs of `cont`, for values that may not be finite (a sliver face whose
// determinant underflows, a NaN vertex): the multiply-by-0 mask of the fast form would turn a neighbouring run's Inf into NaN
// in THIS run, so a wave in which any lane holds a non-finite value takes the select form (two instructions per value and
// step), which keeps a non-finite gradient inside the lanes of the face that produced it, as the reference's per-pair
// atomics do.
template <int N>
__device__ __forceinline__ void seg_scan64_safe(float (&g)[N], unsigned long long cont, int lane) {
    float mag = 0.f;
#pragma unroll
    for (int c = 0; c < N; c++) mag += fabsf(g[c]);
    if (__builtin_expect(__ballot(!(mag < 3.0e38f)) == 0ull, 1)) { seg_scan64_n(g, seg_steps(cont)); return; }
#pragma unroll
    for (int c = 0; c < N; c++) seg_scan64(g[c], cont, lane);
}

}  // namespace dm2
