// One 16-byte chunk of a stored row to f32, by dtype (DT: 0 f32, 1 f16, 2 fp8) -- for the kernels that need a row's
// VALUES rather than a dot product with it (neighbors.h, diverse.h).  Every conversion is exact; fp8 is unscaled.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fp8.h"
#include "gemv_f16.h"

namespace svs {

constexpr int elems_per_chunk(int DT) { return DT == 0 ? 4 : (DT == 1 ? 8 : 16); }

template <int DT>
__device__ __forceinline__ void decode_chunk(u32x4 a, float (&v)[elems_per_chunk(DT)]) {
  const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (DT == 0) {
      v[e] = __uint_as_float(w[e]);
    } else if constexpr (DT == 1) {
      const h2 p = __builtin_bit_cast(h2, w[e]);
      v[2 * e] = (float)p.x;
      v[2 * e + 1] = (float)p.y;
    } else {
      float b[4];
      unpack_fp8x4(w[e], b);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * e + j] = b[j];
    }
  }
}

}  // namespace svs
