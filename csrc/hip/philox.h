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
// Attention-probability dropout (csrc/hip/attention.hip) draws from the same
// generator with its own element assignment, independent of any kernel's
// tiling.  One Philox call serves a patch of 4 queries × 4 keys of one (b, h):
// counter = (g_lo, g_hi, site, step) with the 64-bit patch index
//   g = ((b·H + h)·(S/4) + q/4)·(S/4) + k/4,
// key as above.  Element (q, k) takes output word q % 4, bits 8·(k % 4) …
// 8·(k % 4) + 7, and is kept iff that byte ≥ thr8 = round(p·256): for attention
// p is quantised to 1/256 (1/65536 at the other sites).  Kept probabilities are
// multiplied by scale = 256 / (256 − thr8).  Sites: 0x10000 + layer, disjoint
// from 0 (embedding) and 1 + 2i / 2 + 2i (block i's residual branches).
// A lane of the flash kernels holds one query and runs of 4 consecutive keys
// (forward, dQ) or one key and runs of 4 consecutive queries (dK/dV), so one
// call per lane covers a 32 × 32 score block: the four lanes of a quad each
// draw one of the quad's four patches, reduce it to 16 keep bits
// (attn_patch_keep) and exchange them by DPP quad permutes.  The host reference
// is paddle_operator_amd.ops.core.philox_attn_keep_mask.
//
// DropArgs travels by value as a kernel argument: a captured (graph-replayed)
// step would freeze seed / step / site / offset at their captured values and
// repeat one mask; the GPT-2 step is launched eagerly.
#pragma once
#include <stdint.h>

namespace pdo {

struct DropArgs {
  // 0 = no dropout (callers dispatch to the plain kernels); round(p·65536) at the
  // LayerNorm / embedding sites, thr8 = round(p·256) for attention
  uint32_t thr = 0;
  float scale = 1.f;   // 65536 / (65536 − thr), or 256 / (256 − thr8): fp32, computed on the host
  uint32_t key0 = 0, key1 = 0;  // seed low / high
  uint32_t site = 0, step = 0;
  uint64_t offset = 0;  // added to the group index, in groups of 8 elements (unused by attention)

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
  // attention: thr = thr8 in [0, 255], scale = 256 / (256 − thr8), no offset
  static DropArgs make_attn(uint32_t thr8, uint64_t seed, uint32_t site, uint32_t step) {
    DropArgs d;
    d.thr = thr8;
    d.scale = 256.f / (float)(256u - thr8);
    d.key0 = (uint32_t)seed;
    d.key1 = (uint32_t)(seed >> 32);
    d.site = site;
    d.step = step;
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

// The 16 keep bits of attention patch g: bit 8·kb + w = element (query word w,
// key byte kb) kept.  The four bytes of a word are compared at once: with
// x7 = x & 0x7f per byte, bit 7 of x7 + (0x80 − (thr & 0x7f)) is x7 ≥ thr & 0x7f
// (the sum is at most 0xff: no carry between bytes), and byte ≥ thr is that
// bit OR the byte's own bit 7 for thr < 128, AND for thr ≥ 128.  thr in [1, 255].
__device__ __forceinline__ uint32_t attn_patch_keep(const DropArgs& d, uint64_t g) {
  const Philox4 p = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), d.site, d.step, d.key0, d.key1);
  const uint32_t add = (0x80u - (d.thr & 0x7fu)) * 0x01010101u;
  const uint32_t any = d.thr < 128u ? 0xffffffffu : 0u;
  uint32_t keep = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t x = p.w[w], y = (x & 0x7f7f7f7fu) + add;
    const uint32_t ge = (x & y) | ((x | y) & any);  // bit 7 of every byte
    keep |= (ge & 0x80808080u) >> (7 - w);
  }
  return keep;
}
#endif

}  // namespace pdo
