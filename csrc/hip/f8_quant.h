// SPDX-License-Identifier: Apache-2.0
// The power-of-two e4m3 scale rule and the 8-value convert shared by the per-tensor
// quantiser (quant_f8.hip) and the LayerNorm forward that writes e4m3 rows
// (layernorm.hip).  The rule itself: quant_f8.hip's head.
#pragma once
#include "common.h"

namespace pdo {

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

// e of s = 2^e from the bits of amax = m·2^a: 8 − a for m ≤ 1.75, else 7 − a; 0 for amax = 0; |e| ≤ 126
__device__ __forceinline__ int f8_scale_exp(unsigned amax_bits) {
  if (amax_bits == 0u) return 0;
  const int a = (int)(amax_bits >> 23) - 127;
  const int e = ((amax_bits & 0x7fffffu) <= 0x600000u ? 8 : 7) - a;
  return e < -126 ? -126 : e > 126 ? 126 : e;
}

// 2^e as a float, |e| ≤ 126
__device__ __forceinline__ float f8_pow2(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }

// 8 floats → 8 e4m3 bytes (v_cvt_pk_fp8_f32, RNE, OCP e4m3fn on gfx950)
__device__ __forceinline__ i32x2 f8_cvt8(f32x8 f) {
  i32x2 o = {0, 0};
  o[0] = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], o[0], false);
  o[0] = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], o[0], true);
  o[1] = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], o[1], false);
  o[1] = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], o[1], true);
  return o;
}

}  // namespace pdo
