// The dead-row bitmap (svs_index_mask_rows): bit r & 31 of word r >> 5 is set when local row r is tombstoned.  Its
// layout is spelled out here and nowhere else on the device; a null bitmap means that no row is masked.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svs {

__device__ __forceinline__ bool row_dead(const uint32_t* bits, int64_t r) {
  return bits && ((bits[r >> 5] >> (uint32_t)(r & 31)) & 1u);
}

// Bits 0 .. 3: rows 4 i4 .. 4 i4 + 3, which share one word (the bits above them belong to the rows that follow)
__device__ __forceinline__ uint32_t dead_nibble(const uint32_t* bits, int64_t i4) {
  return bits ? bits[i4 >> 3] >> ((uint32_t)(i4 & 7) * 4u) : 0u;
}

}  // namespace svs
