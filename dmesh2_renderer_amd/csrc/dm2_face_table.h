// dm2_face_table.h -- per-block LDS table keyed by face id, the gradient scatter of the layer kernels
// (k_layer_composite_bwd, k_layer_composite<WEIGHTS>, k_rasterize_bwd).
//
// A (pixel, face) contribution adds its components into the face's slot; the block then flushes the table with one global
// atomic per (face or vertex row, component) and face of the tile (MI355X: 64 lanes adding into 64 different rows run ~17x
// below the chip's atomic rate).  A face that finds no slot within LC_PROBES probes adds straight to global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dm2 {

constexpr int LC_SLOTS = 512;      // LDS accumulator slots (distinct faces) per tile
constexpr int LC_PROBES = 16;

// slot of face f in the tile's table (inserted if new), -1 when LC_PROBES probes find neither f nor a free slot
__device__ __forceinline__ int lc_slot(int* keys, int f) {
    const uint32_t h = ((uint32_t)f * 2654435761u) >> 23;          // 9 bits: LC_SLOTS = 512
#pragma unroll 1
    for (int p = 0; p < LC_PROBES; p++) {
        const int s = (int)((h + (uint32_t)p) & (LC_SLOTS - 1));
        const int old = atomicCAS(&keys[s], -1, f);
        if (old == -1 || old == f) return s;
    }
    return -1;
}

}  // namespace dm2
