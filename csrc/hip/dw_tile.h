// SPDX-License-Identifier: Apache-2.0
// The token-major LDS tile of the weight-gradient GEMMs (gemm_dw.hip,
// gemm_dw4.hip): [BK tokens][LROW elements] bf16 as it lies in memory, 16-B
// chunk index XOR (token & 3)·4 so the transposed reads of 4 token rows × 64 B
// per half-wave hit 4 distinct 64-B bank groups, read as 32x32x16 MFMA
// operands with the transposing LDS read.
#pragma once
#include "cdna4.h"

namespace pdo {

template <int LROW>
struct DwTile {
  // element offset of (token row r, 16-B chunk ch) in the swizzled LDS tile
  static __device__ __forceinline__ int loff(int r, int ch) { return r * LROW + ((ch ^ ((r & 3) << 2)) << 3); }

  // per-lane element offset of the transposed fragment for k0 = 0 and columns
  // [cb, cb + 32); tokens k0 + 4·(lane>>5) + q and +8 (q = (lane>>2)&3)
  static __device__ __forceinline__ int frag_base(int cb, int lane) {
    const int g = lane >> 4, t = lane & 15, q = t >> 2, p = t & 3;
    const int col = cb + 16 * (g & 1) + 4 * p;
    const int r0 = 4 * (g >> 1) + q;
    return loff(r0, col >> 3) + (col & 7);
  }

  // the fragment of tokens [K0, K0 + 16) at T = tile + frag_base(cb, lane)
  template <int K0>
  static __device__ __forceinline__ bf16x8 frag(const bf16* T) {
    return ld_tr8(T + K0 * LROW, T + (K0 + 8) * LROW);
  }
};

}  // namespace pdo
