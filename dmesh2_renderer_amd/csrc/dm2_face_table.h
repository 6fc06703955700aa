// dm2_face_table.h -- FaceTable: the per-block LDS table of the scatter kernels, one lane per pixel of a 16 x 16 tile
// (k_layer_composite<WEIGHTS>, k_layer_composite_bwd, k_rasterize_bwd, k_interpolate_bwd_attr, k_texture_bwd_tex, k_composite_bwd<FACE>, k_coverage_bwd, and through
// dm2_tex_core.h's tex_scatter_layer k_texture_mip_bwd_tex, k_texture_cube_bwd_tex).  DESIGN.md 8, "The face table".
//
// Neighbouring pixels list the same faces (or texels).  A (pixel, key) contribution adds its components into the key's slot,
// and the block then flushes with one global atomic per (key, component) of the tile rather than one per (pixel, key,
// component): on MI355X 64 lanes adding into 64 different rows run ~17x below the chip's atomic rate.  Float atomics, in LDS
// as in global memory, leave the last bits of a sum to the order of the run.
// Overflow: when slot() finds neither the key nor a free slot in LC_PROBES probes it returns -1, and the caller adds that
// contribution straight to global memory: the table is an accelerator, never a bound on what a tile may list.
// Layout: component-major, acc[c * STRIDE + slot]; a padded STRIDE spreads the components of one slot over the banks.
// Flush: every (slot, component) pair goes to one lane, which skips an empty slot and a sum that is exactly zero and hands
// (key, component, sum) to the kernel's callback.  flush_by_component: consecutive lanes on consecutive slots of a component.
// flush_by_slot: consecutive lanes on the components of one slot, where those are neighbours in global memory (one row's channels).
// Barriers are the kernel's: after clearing, before a flush, and between a flush and the next clear_acc() (keys may stay).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dm2_device_math.h"

namespace dm2 {

constexpr int LC_SLOTS = 512;      // LDS accumulator slots (distinct faces) per tile
constexpr int LC_PROBES = 16;

constexpr int LC_HASH_SHIFT = 32 - __builtin_ctz(LC_SLOTS);                // the hash keeps the product's top log2(LC_SLOTS) bits
static_assert(LC_SLOTS > 1 && (LC_SLOTS & (LC_SLOTS - 1)) == 0, "LC_SLOTS is a power of two: the hash and the probe's wrap");

// Trivially constructible: declare it __shared__.  The clearing and flush loops stride by TILE_PIX: the kernel is launched
// with blockDim.x == TILE_PIX and passes tid = threadIdx.x.
template <typename T, int NCOMP, int STRIDE = LC_SLOTS>
struct alignas(16) FaceTable {
    static_assert(STRIDE >= LC_SLOTS, "STRIDE pads the LC_SLOTS slots of a component, it cannot cut them");
    int key[LC_SLOTS];             // -1: free
    alignas(16) T acc[NCOMP * STRIDE];
    __device__ __forceinline__ void clear_keys(int tid) { for (int i = tid; i < LC_SLOTS; i += TILE_PIX) key[i] = -1; }
    __device__ __forceinline__ void clear_acc(int tid) { for (int i = tid; i < NCOMP * STRIDE; i += TILE_PIX) acc[i] = T(0); }
    __device__ __forceinline__ void clear(int tid) {                       // both, in one sweep
        for (int i = tid; i < NCOMP * STRIDE; i += TILE_PIX) { if (i < LC_SLOTS) key[i] = -1; acc[i] = T(0); }
    }
    // slot of key k >= 0 (inserted if new), -1 when LC_PROBES probes find neither k nor a free slot
    __device__ __forceinline__ int slot(int k) {
        const uint32_t h = ((uint32_t)k * 2654435761u) >> LC_HASH_SHIFT;
#pragma unroll 1
        for (int p = 0; p < LC_PROBES; p++) {
            const int s = (int)((h + (uint32_t)p) & (LC_SLOTS - 1));
            const int old = atomicCAS(&key[s], -1, k);
            if (old == -1 || old == k) return s;
        }
        return -1;
    }
    __device__ __forceinline__ void add(int s, int c, T v) { atomicAdd(&acc[c * STRIDE + s], v); }
    // add() for s >= 0, *global for the overflow route, as one atomic on a selected address.  For k_layer_composite<.., true>
    // alone: its blend loop measured slower with the branch the other kernels use (profiles/face_table_ab.txt).
    __device__ __forceinline__ void add_or(int s, int c, T v, T* global) { atomicAdd(s >= 0 ? &acc[c * STRIDE + s] : global, v); }

    // fn(key, c, sum) for every held key's components with a non-zero sum
    template <typename F>
    __device__ __forceinline__ void flush_by_slot(int tid, F&& fn) const {          // lane -> (slot, c), c fastest
        for (int i = tid; i < NCOMP * LC_SLOTS; i += TILE_PIX) flush_one(i / NCOMP, i % NCOMP, fn);
    }
    template <typename F>
    __device__ __forceinline__ void flush_by_component(int tid, F&& fn) const {     // lane -> (c, slot), slot fastest
        for (int i = tid; i < NCOMP * LC_SLOTS; i += TILE_PIX) flush_one(i % LC_SLOTS, i / LC_SLOTS, fn);
    }

private:
    template <typename F>
    __device__ __forceinline__ void flush_one(int s, int c, F&& fn) const {
        const int k = key[s];
        if (k < 0) return;
        const T v = acc[c * STRIDE + s];
        if (v == T(0)) return;
        fn(k, c, v);
    }
};

// lane tid's pixel of the block's 16 x 16 tile, the view on blockIdx.z; pix: its index in (B, H, W), of use when inside
struct TilePixel { uint32_t px, py; bool inside; int64_t pix; };
__device__ __forceinline__ TilePixel tile_pixel(int tid, int W, int H) {
    const uint32_t px = blockIdx.x * TILE + (tid & 15), py = blockIdx.y * TILE + (tid >> 4);
    return {px, py, (px < (uint32_t)W) && (py < (uint32_t)H), ((int64_t)blockIdx.z * H + py) * W + px};
}

// the launch grid of one block per 16 x 16 tile and view
inline dim3 tile_grid(int W, int H, int B) { return dim3((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, B); }

}  // namespace dm2
