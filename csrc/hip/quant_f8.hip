// SPDX-License-Identifier: Apache-2.0
// Per-tensor, power-of-two, just-in-time e4m3 quantisation of a bf16 matrix
// (rows with a stride, so a weight slice or an activation view needs no copy).
// Two passes and no state: amax_bf16 leaves max |x| in one device word,
// quant_e4m3 derives the scale from it in every workgroup and converts.
//
// amax: |x| of a finite bf16 orders like its 15 low bits as an integer, so the
// maximum is taken on the bit patterns (v_pk_max_u16, 8 values per 16-B load)
// and lands with one vector atomicMax per wave on the float's bit pattern —
// order-independent, hence deterministic.  The word is cleared by a one-lane
// kernel in front (stream-ordered; a memset node is avoided so the pair may be
// captured into a graph).
//
// Scale s = 2^e from amax = m·2^a, m ∈ [1, 2): e = 8 − a for m ≤ 1.75, else
// 7 − a, so amax·s ∈ (224, 448] (448 = the largest finite e4m3).  e comes from
// the exponent and mantissa BITS (f8_scale_exp, f8_quant.h), which a host reference
// reproduces exactly; amax = 0 → e = 0; e is clamped to ±126 so s and 1/s are
// normal.  x·s is exact in fp32 and the hardware convert (v_cvt_pk_fp8_f32,
// OCP e4m3fn on gfx950) rounds to nearest even: 16 B of bf16 in, 8 B of fp8 out
// per lane.  Only finite inputs are specified.
#include "common.h"
#include "f8_quant.h"
#include "kernels.h"

namespace pdo {

namespace {

constexpr int NTHR = 256;
// vector v of the matrix → element offsets in x (stride ld) and q (stride ldq)
struct RowMap {
  unsigned vpr;  // 16-B vectors per row
  long long ld, ldq;
  __device__ __forceinline__ void at(unsigned v, long long& xo, long long& qo) const {
    const unsigned r = v / vpr, c = v - r * vpr;
    xo = r * ld + 8ll * c;
    qo = r * ldq + 8ll * c;
  }
};

__global__ void amax_clear_kernel(unsigned* out) { *out = 0u; }

// nvec = rows · vpr 16-B vectors; tail = cols % 8 trailing elements (rows = 1 only)
__global__ __launch_bounds__(NTHR) void amax_bf16_kernel(const bf16* __restrict__ x, unsigned nvec, RowMap rm, int tail,
                                                         unsigned* __restrict__ out) {
  u16x8 m = {0, 0, 0, 0, 0, 0, 0, 0};
  for (unsigned v = blockIdx.x * NTHR + threadIdx.x; v < nvec; v += gridDim.x * NTHR) {
    long long xo, qo;
    rm.at(v, xo, qo);
    const u16x8 b = *reinterpret_cast<const u16x8*>(x + xo);
    m = __builtin_elementwise_max(m, b & (unsigned short)0x7fff);
  }
  unsigned r = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) r = max(r, (unsigned)m[k]);
  if (blockIdx.x == 0 && (int)threadIdx.x < tail)
    r = max(r, (unsigned)(reinterpret_cast<const unsigned short*>(x)[8ll * nvec + threadIdx.x] & 0x7fff));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r = max(r, (unsigned)__shfl_xor((int)r, o, 64));
  if ((threadIdx.x & 63) == 0 && r) atomicMax(out, r << 16);
}

__global__ __launch_bounds__(NTHR) void quant_e4m3_kernel(const bf16* __restrict__ x, unsigned nvec, RowMap rm, int tail,
                                                          const unsigned* __restrict__ amax,
                                                          unsigned char* __restrict__ q, float* __restrict__ dscale) {
  const int e = f8_scale_exp(*amax);
  const float s = __uint_as_float((unsigned)(127 + e) << 23);
  if (blockIdx.x == 0 && threadIdx.x == 0) *dscale = __uint_as_float((unsigned)(127 - e) << 23);
  for (unsigned v = blockIdx.x * NTHR + threadIdx.x; v < nvec; v += gridDim.x * NTHR) {
    long long xo, qo;
    rm.at(v, xo, qo);
    const f32x8 f = to_f32(*reinterpret_cast<const bf16x8*>(x + xo)) * s;
    *reinterpret_cast<i32x2*>(q + qo) = f8_cvt8(f);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
    const long long i = 8ll * nvec + threadIdx.x;
    const float f = (float)x[i] * s;
    q[i] = (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(f, 0.f, 0, false) & 0xff);
  }
}

// rows > 1: whole 16-B vectors per row and aligned row starts; one row: any length
bool shape_ok(long long rows, long long cols, long long ld, long long ldq) {
  if (rows < 1 || cols < 1 || ld < cols || ldq < cols) return false;
  if (rows > 1 && (cols % 8 || ld % 8 || ldq % 8)) return false;
  return rows * ((cols + 7) / 8) < (1ll << 31);
}

struct Launch {
  unsigned nvec;
  RowMap rm;
  int tail, grid;
};
Launch plan(long long rows, long long cols, long long ld, long long ldq) {
  if (ld == cols && ldq == cols) {  // contiguous: one long row
    cols *= rows;
    rows = 1;
  }
  const long long vpr = cols / 8, nvec = rows * vpr;
  return {(unsigned)nvec, RowMap{(unsigned)(vpr ? vpr : 1), ld, ldq}, (int)(cols % 8), stream_grid(nvec, NTHR * 4)};
}

}  // namespace

int amax_bf16(const bf16* x, long long rows, long long cols, long long ld, unsigned* amax_out, hipStream_t st) {
  if (!shape_ok(rows, cols, ld, cols)) return -2;
  const Launch l = plan(rows, cols, ld, cols);
  amax_clear_kernel<<<1, 1, 0, st>>>(amax_out);
  amax_bf16_kernel<<<l.grid, NTHR, 0, st>>>(x, l.nvec, l.rm, l.tail, amax_out);
  return 0;
}

int quant_e4m3(const bf16* x, long long rows, long long cols, long long ld, const unsigned* amax, unsigned char* q,
               long long ldq, float* dscale_out, hipStream_t st) {
  if (!shape_ok(rows, cols, ld, ldq)) return -2;
  const Launch l = plan(rows, cols, ld, ldq);
  quant_e4m3_kernel<<<l.grid, NTHR, 0, st>>>(x, l.nvec, l.rm, l.tail, amax, q, dscale_out);
  return 0;
}

}  // namespace pdo
