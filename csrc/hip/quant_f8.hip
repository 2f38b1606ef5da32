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
//
// Grouped form (quant_e4m3_grouped): the same two passes over a TABLE of segments of
// one bf16 arena — the step's FP8 weights, quantised once per optimizer step instead
// of three small launches in front of every GEMM — into one compact byte arena, with
// one amax word and one scale per segment.  Three launches for any number of tensors:
// clear the n amax words, amax, convert.
//
// Split of the work: one workgroup per CHUNK (GCH = 8192 elements, 16 KiB of bf16) of
// one tensor, not a persistent grid-stride loop.  A chunk never spans two tensors, so
// a workgroup finds its table row once (binary search on the first-chunk column, as
// transpose_bf16_batched does), reduces to ONE amax word and needs no per-vector row
// lookup; a grid-stride loop over chunks would repeat the search and the LDS reduction
// per chunk to save only the workgroup launch, which at 16 KiB in and 8 KiB out per
// workgroup is small beside the traffic.  GPT-2-medium's sets are 20,480 ("ln") to
// 32,256 ("lnmx") chunks: ≥ 80 workgroups per CU, so the tail is short.  Each lane
// issues its four 16-B loads (one per 256-lane stripe of the chunk, coalesced) before
// the first use; vectors past the tensor's end (only in its last chunk) are skipped.
// amax: packed u16 max per lane → wave (shuffles) → workgroup (4 words of LDS) → one
// atomicMax per workgroup.  Nothing waits on another workgroup inside a launch; the
// convert launch reads the finished amax words.  The convert workgroup of a tensor's
// chunk 0 writes its 2^−e.  Same f8_scale_exp and f8_cvt8 on the same bf16 values as
// the per-tensor pair, and a max is order-free: the bytes and scales are identical.
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

// ---- grouped form: a table of arena segments, one workgroup per chunk (file header) ----
constexpr int GCH = QUANT_GROUP_CHUNK;  // elements per chunk
constexpr int GVC = GCH / 8;            // 16-B vectors per chunk
constexpr int GLD = GVC / NTHR;         // 16-B loads per lane, all issued before the first use
static_assert(GLD * NTHR * 8 == GCH && GLD >= 2, "a chunk is a whole number of 256-lane stripes");

__global__ void clear_words_kernel(unsigned* p, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}

// what chunk b covers: its tensor t (the row whose first chunk is the last one ≤ b), the tensor's element offsets
// in the bf16 and the byte arena, the chunk's first 16-B vector inside the tensor and the tensor's vector count
struct Seg {
  int t;
  long long src, dst, v0, nvec;
};
__device__ __forceinline__ Seg find_seg(const long long* __restrict__ table, int n, long long b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[4 * mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const long long* e = table + 4 * lo;
  return {lo, e[1], e[2], (b - e[0]) * GVC, e[3] / 8};
}

// the lane's GLD vectors of the chunk (stripe i: vector v0 + i·NTHR + lane); zeros past the tensor's end
template <typename V>
__device__ __forceinline__ void load_chunk(const V* __restrict__ x, const Seg& s, V (&b)[GLD]) {
  const long long v = s.v0 + threadIdx.x;
  if (s.v0 + GVC <= s.nvec) {  // a whole chunk (uniform branch): unconditional loads, back to back
#pragma unroll
    for (int i = 0; i < GLD; ++i) b[i] = x[v + i * NTHR];
  } else {
#pragma unroll
    for (int i = 0; i < GLD; ++i) b[i] = v + i * NTHR < s.nvec ? x[v + i * NTHR] : V{};
  }
}

__global__ __launch_bounds__(NTHR) void amax_grouped_kernel(const bf16* __restrict__ src,
                                                            const long long* __restrict__ table, int n,
                                                            unsigned* __restrict__ amax) {
  __shared__ unsigned red[NTHR / WAVE];
  const Seg s = find_seg(table, n, blockIdx.x);
  u16x8 b[GLD];
  load_chunk(reinterpret_cast<const u16x8*>(src + s.src), s, b);
  u16x8 m = b[0] & (unsigned short)0x7fff;
#pragma unroll
  for (int i = 1; i < GLD; ++i) m = __builtin_elementwise_max(m, b[i] & (unsigned short)0x7fff);
  unsigned r = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) r = max(r, (unsigned)m[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r = max(r, (unsigned)__shfl_xor((int)r, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < NTHR / WAVE; ++w) r = max(r, red[w]);
    if (r) atomicMax(amax + s.t, r << 16);
  }
}

__global__ __launch_bounds__(NTHR) void quant_grouped_kernel(const bf16* __restrict__ src,
                                                             const long long* __restrict__ table, int n,
                                                             const unsigned* __restrict__ amax,
                                                             unsigned char* __restrict__ q, float* __restrict__ dscale) {
  const Seg s = find_seg(table, n, blockIdx.x);
  bf16x8 b[GLD];
  load_chunk(reinterpret_cast<const bf16x8*>(src + s.src), s, b);
  const int e = f8_scale_exp(amax[s.t]);
  const float sc = f8_pow2(e);
  if (s.v0 == 0 && threadIdx.x == 0) dscale[s.t] = f8_pow2(-e);
  i32x2* out = reinterpret_cast<i32x2*>(q + s.dst);
  const long long v = s.v0 + threadIdx.x;
#pragma unroll
  for (int i = 0; i < GLD; ++i)
    if (v + i * NTHR < s.nvec) out[v + i * NTHR] = f8_cvt8(to_f32(b[i]) * sc);
}

}  // namespace

int quant_e4m3_grouped(const bf16* src, long long src_n, unsigned char* q, long long q_n, unsigned* amax, float* dscale,
                       const long long* table_dev, const long long* table_host, int n, long long chunks,
                       hipStream_t st) {
  if (n < 1 || chunks < 1 || chunks > 0x7fffffffLL) return -2;
  long long want = 0;
  for (const long long* e = table_host; e != table_host + 4ll * n; e += 4) {
    if (e[0] != want || e[3] < 8 || e[3] % 8 || e[1] % 8 || e[2] % 8) return -2;
    if (e[1] < 0 || e[1] > src_n - e[3] || e[2] < 0 || e[2] > q_n - e[3]) return -3;
    want += (e[3] + GCH - 1) / GCH;
  }
  if (want != chunks) return -2;
  clear_words_kernel<<<(n + NTHR - 1) / NTHR, NTHR, 0, st>>>(amax, n);
  amax_grouped_kernel<<<(unsigned)chunks, NTHR, 0, st>>>(src, table_dev, n, amax);
  quant_grouped_kernel<<<(unsigned)chunks, NTHR, 0, st>>>(src, table_dev, n, amax, q, dscale);
  return 0;
}

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
