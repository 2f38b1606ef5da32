// SPDX-License-Identifier: Apache-2.0
// Counter-based dropout masks (Philox4x32-10) for the LayerNorm and embedding
// kernels.  No mask is stored: the keep decision of an element is a pure
// function of (seed, step, site, element index), generated in the forward and
// regenerated in the backward.
//
// One Philox call serves a group of 8 consecutive bf16 elements (one 16-B
// vector).  key = (low, high) 32 bits of the 64-bit seed; counter =
// (g_lo, g_hi, site, step) with g = offset + row·(C/8) + c8 the group's index
// in the flattened [T, C] tensor.  Element j of the group takes output word
// j >> 1, bits 0-15 for even j and bits 16-31 for odd j, and is kept iff that
// 16-bit value ≥ thr = round(p·65536): p is quantised to 1/65536.  Kept values
// are multiplied by scale = 65536 / (65536 − thr).  The host reference is
// paddle_operator_amd.ops.core.philox_keep_mask.
//
// DropArgs travels by value as a kernel argument: a captured (graph-replayed)
// step would freeze seed / step / site / offset at their captured values and
// repeat one mask; the GPT-2 step is launched eagerly.
#pragma once
#include <stdint.h>

namespace pdo {

struct DropArgs {
  uint32_t thr = 0;    // 0 = no dropout (callers dispatch to the plain kernels)
  float scale = 1.f;   // 65536 / (65536 − thr), fp32, computed on the host
  uint32_t key0 = 0, key1 = 0;  // seed low / high
  uint32_t site = 0, step = 0;
  uint64_t offset = 0;  // added to the group index, in groups of 8 elements

  static DropArgs make(uint32_t thr, uint64_t seed, uint32_t site, uint32_t step, uint64_t offset) {
    DropArgs d;
    d.thr = thr;
    d.scale = 65536.f / (float)(65536u - thr);
    d.key0 = (uint32_t)seed;
    d.key1 = (uint32_t)(seed >> 32);
    d.site = site;
    d.step = step;
    d.offset = offset;
    return d;
  }
};

#if defined(__HIPCC__)
struct Philox4 {
  uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// keep bits of group g (bit j = element j kept)
__device__ __forceinline__ uint32_t drop_keep_bits(const DropArgs& d, uint64_t g) {
  g += d.offset;
  const Philox4 p = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), d.site, d.step, d.key0, d.key1);
  uint32_t keep = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t v = (j & 1) ? (p.w[j >> 1] >> 16) : (p.w[j >> 1] & 0xFFFFu);
    keep |= (v >= d.thr ? 1u : 0u) << j;
  }
  return keep;
}
#endif

}  // namespace pdo
