// SPDX-License-Identifier: Apache-2.0
// The token-major LDS tile of the weight-gradient GEMMs (gemm_dw.hip,
// gemm_dw4.hip): [BK tokens][LROW elements] bf16 as it lies in memory, with the
// 16-B chunk index of a token row XORed by swz(row), read as MFMA operands with
// the transposing LDS read.  Two layouts, one per MFMA shape; both have
//   swz(r)              the chunk XOR of token row r
//   loff(r, ch)         element offset of (token row r, 16-B chunk ch)
//   frag_base(cb, lane) per-lane element offset of the fragment of columns cb ..
//   frag<K0>(T)         the fragment of tokens K0 .. at T = tile + frag_base(cb, lane)
#pragma once
#include "cdna4.h"

namespace pdo {

// 32x32x16 operands: chunk XOR (token & 3)·4, so the transposed reads of 4 token
// rows × 64 B per half-wave hit 4 distinct 64-B bank groups.
template <int LROW>
struct DwTile {
  static __device__ __forceinline__ int swz(int r) { return (r & 3) << 2; }
  static __device__ __forceinline__ int loff(int r, int ch) { return r * LROW + ((ch ^ swz(r)) << 3); }

  // columns [cb, cb + 32) at k0 = 0; tokens k0 + 4·(lane>>5) + q and +8 (q = (lane>>2)&3)
  static __device__ __forceinline__ int frag_base(int cb, int lane) {
    const int g = lane >> 4, t = lane & 15, q = t >> 2, p = t & 3;
    const int col = cb + 16 * (g & 1) + 4 * p;
    const int r0 = 4 * (g >> 1) + q;
    return loff(r0, col >> 3) + (col & 7);
  }

  // tokens [K0, K0 + 16)
  template <int K0>
  static __device__ __forceinline__ bf16x8 frag(const bf16* T) {
    return ld_tr8(T + K0 * LROW, T + (K0 + 8) * LROW);
  }
};

// 16x16x32 operands.  Lane group g = l >> 4 reads 4 token rows 4g .. 4g+3 (lo) and
// 16 + 4g .. (hi) of the 16 columns cb .. cb+15, so lane l holds column
// cb + (l & 15) at tokens {4g..4g+3, 16+4g..16+4g+3} — a k permutation shared by
// both operands.  The 16 rows a wave reads per instruction pair up as lane groups
// {0,1} / {2,3} (or {0,2} / {1,3}); with the swizzle above rows r and r + 4 would
// hit the same banks, so this one XORs the 32-B column pair index with
// (r & 3) | bit2 = b2(r) ^ b3(r): 8 distinct bank octets for either pairing.  A
// DMA's source-side swizzle then depends on row bit 3.
template <int LROW>
struct DwTile16 {
  static __device__ __forceinline__ int swz(int r) { return ((r & 3) | ((((r >> 2) ^ (r >> 3)) & 1) << 2)) << 1; }
  static __device__ __forceinline__ int loff(int r, int ch) { return r * LROW + ((ch ^ swz(r)) << 3); }

  // columns [cb, cb + 16) at k0 = 0
  static __device__ __forceinline__ int frag_base(int cb, int lane) {
    const int g = lane >> 4, t = lane & 15, q = t >> 2, p = t & 3;
    const int col = cb + 4 * p;
    return loff(4 * g + q, col >> 3) + (col & 7);
  }

  // tokens [K0, K0 + 32)
  template <int K0>
  static __device__ __forceinline__ bf16x8 frag(const bf16* T) {
    return ld_tr8(T + K0 * LROW, T + (K0 + 16) * LROW);
  }
};

}  // namespace pdo
