// SPDX-License-Identifier: Apache-2.0
// gfx950 (CDNA4) primitives shared by the MFMA kernels: attention.hip, conv.hip,
// gemm_nt.hip, gemm_nt4.hip, gemm_dw.hip and gemm_dw4.hip.  Each statement whose
// slip gives wrong numbers on some waves without a fault exists once, here, with
// its contract; the kernels keep only the reason why they may use a given form.
//
// hipcc does not look inside an asm string: it neither counts the memory
// operations in it (the caller waits with vm_wait) nor pads its hazards (every
// wait state an instruction inside needs is inside the string).
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace pdo {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;  // operand type of the transposing LDS read

// f(integral_constant<int, I>) for I = 0 .. N-1, expanded at compile time: every
// index is a constant (a 128-slot MFMA schedule is too large for `#pragma
// unroll`: hipcc gives up and indexes the accumulators at run time)
template <typename Fn, int... I>
__device__ __forceinline__ void static_for_impl(Fn&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename Fn>
__device__ __forceinline__ void static_for(Fn&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// LDS byte address of a pointer into __shared__ memory (what M0 and the
// ds_* instructions take); p must point into LDS
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}

// ---- LDS-DMA: global → LDS without register staging.  One wave-instruction
// writes lane l's 16 B (4 B for glds4) to LDS byte lds_byte + 16·l (4·l): the
// image is lane-linear, so a swizzle goes on the SOURCE address.  lds_byte is
// wave-uniform and travels in M0; `s_nop 0` is the wait state between the SALU
// write of M0 and the DMA that reads it.  The DMA counts in vmcnt, in order with
// the wave's other vector memory operations, and hipcc does not see it: the
// consumer waits with vm_wait<N>() for its own pieces, then passes a barrier,
// then reads (__syncthreads() alone does not wait for it).
//
// glds16 / glds4 / bufld16_lds leave M0 changed.  A kernel may use them only if
// nothing else in it reads M0 between DMAs: no LDS instruction that takes M0
// (ds_*_addtid, ds_gws_*), no s_movrel / v_interp, no readlane-by-M0, and no
// builtin LDS-DMA next to the asm one.  After editing such a kernel, look for
// other M0 readers in its assembly (hipcc -S).
//
// source = sbase (wave-uniform, SGPR pair) + voff (per lane, bytes, 32-bit unsigned)
__device__ __forceinline__ void glds16(unsigned voff, const void* sbase, unsigned lds_byte) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_byte)
               : "memory");
}
__device__ __forceinline__ void glds4(unsigned voff, const void* sbase, unsigned lds_byte) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_byte)
               : "memory");
}
// The same 16-B DMA from a per-lane 64-bit pointer, with M0 saved and restored
// in the statement (two more SALU moves per DMA): safe next to anything hipcc
// does with M0, no audit of the assembly needed.  The 8-wave kernels (gemm_nt,
// gemm_dw) use this form; their per-lane sources are pointers already.
__device__ __forceinline__ void glds16_keep_m0(const void* src, unsigned lds_byte) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(lds_byte)
               : "memory");
}
// 16-B DMA through a buffer descriptor (buf_rsrc): a lane whose voff is ≥ the
// descriptor's byte count writes zeros to LDS — padding without a zero-fill
// pass.  M0 is not preserved (rule above).
__device__ __forceinline__ void bufld16_lds(unsigned voff, __amdgpu_buffer_rsrc_t rs, unsigned lds_byte) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(rs),
               "s"(lds_byte)
               : "memory");
}

// Raw buffer descriptor over [p, p + bytes): stride 0, so the range check is
// "byte offset < bytes" (out of range: loads return 0, stores are dropped).
// BUF_RAW32 is descriptor word 3 with only DATA_FORMAT (bits 18:15) = 4, a
// 32-bit element: no swizzle, no index stride, no ADD_TID — the value raw dword
// buffers take on gfx90a / gfx942 / gfx950.  p and bytes must be wave-uniform.
constexpr int BUF_RAW32 = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, BUF_RAW32);
}

// wait until at most N of this wave's vector memory operations (LDS-DMA
// included) are outstanding; they retire in issue order
template <int N>
__device__ __forceinline__ void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Transposing LDS read (ds_read_b64_tr_b16): 4 bf16 of one column from 4
// consecutive rows of the 16 × 16 block the lane group addresses.  p is this
// lane's address: 8-B aligned, in LDS.
__device__ __forceinline__ bf16x4 ld_tr4(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p);
}
__device__ __forceinline__ bf16x8 cat8(bf16x4 lo, bf16x4 hi) {
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// The pair of them as one MFMA operand; lo_p / hi_p are this lane's addresses
// in the two row groups (8 rows apart for 32x32x16, 16 for 16x16x32).  Both
// addresses are formed before the first read; a kernel whose code depends on
// "address, read, address, read" writes cat8(ld_tr4(a), ld_tr4(b)) in two
// statements (attention.hip tr_frag).
__device__ __forceinline__ bf16x8 ld_tr8(const void* lo_p, const void* hi_p) {
  const bf16x4 lo = ld_tr4(lo_p);
  const bf16x4 hi = ld_tr4(hi_p);
  return cat8(lo, hi);
}

// XCD remap of a workgroup id: the hardware deals ids round-robin over the 8
// XCDs, so ids b and b + 8 share an XCD (and its L2).  Returns the logical id
// that gives each XCD a contiguous range of [0, nwg); bijective for any nwg,
// 0 ≤ id < nwg.  The long long form is conv.hip's (its statement order differs
// on purpose: it keeps that kernel's scalar prologue as it was).
__device__ __forceinline__ int xcd_remap(int id, int nwg) {
  const int xcd = id & 7, slot = id >> 3, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}
__device__ __forceinline__ long long xcd_remap(long long id, long long nwg) {
  const long long q = nwg >> 3, r = nwg & 7, x = id & 7, slot = id >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + slot;
}

// q = x / d, r = x - q·d for 0 ≤ x < 2^24 and inv = 1.f / d (exact: the float
// product is off by at most one, which the correction takes back)
__device__ __forceinline__ void divmod(int x, int d, float inv, int& q, int& r) {
  q = (int)((float)x * inv);
  r = x - q * d;
  if (r < 0) {
    --q;
    r += d;
  } else if (r >= d) {
    ++q;
    r -= d;
  }
}

// v_mfma_f32_32x32x16_bf16 through the builtin (hipcc allocates and pads it)
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
__device__ __forceinline__ f32x16 bcast16(float v) {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = v;
  return z;
}

// v_mfma_f32_16x16x32_bf16 with the accumulator pinned to the accumulator file
// ("a"): for kernels whose 256 accumulators per lane fill it (gemm_nt4,
// gemm_dw4), where the builtin made hipcc shuttle them through arch VGPRs.
// Nothing is padded: the operands must come from loads hipcc counts (ds_read),
// an accumulator's first write is mfma16_acc0 (C = 0: no v_accvgpr_write a
// following MFMA would read too early), it is rewritten only as the whole C of a
// later MFMA, and the epilogue pads 16 wait states before v_accvgpr_read.
__device__ __forceinline__ void mfma16_acc(f32x4& c, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16_acc0(f32x4& c, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(c) : "v"(a), "v"(b));
}
// the same pair for v_mfma_f32_32x32x16_bf16, under the same rules (gemm_dw4)
__device__ __forceinline__ void mfma32_acc(f32x16& c, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma32_acc0(f32x16& c, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=a"(c) : "v"(a), "v"(b));
}

}  // namespace pdo
