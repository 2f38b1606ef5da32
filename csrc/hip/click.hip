// SPDX-License-Identifier: Apache-2.0
// Click-log batches for the CTR trainer (gfx950): the record sampler of
// paddle_operator_amd/data.py (CLICK_DOC), the per-slot hash of the raw categorical
// values into table rows, the min–max normalise of the dense features and the fp32
// label, one launch.
//
// cat is [n][S] uint32 (raw values), dense [n][n_dense] int32 (INT_MIN = missing),
// label [n] uint8, stats [2][n_dense] fp32 (row 0 min, row 1 diff > 0).  The outputs
// are ids int64 [B][S], dense_out fp32 [B][n_dense] and label_out fp32 [B].  Row j of
// batch m is global row g = row0 + j (row0 = rank·B, g < 2³²).  Staged: cat / dense /
// label are [B][…] buffers gathered on the host and row j reads entry j; the record
// is drawn here all the same (pad rows are known), so both routes write the same bits.
//
// Draw; key = (low, high) words of the data seed (host reference: data.record_index):
//   stream 0 (training):   philox(g, 0, stream, m) → i = ((w1 << 32) | w0) mod n
//   stream 1 (evaluation): i = m·Bglobal + g, not random; a row with i ≥ n is a pad
//   row: every id −1, every dense value +0.0, label −1, rec_out −1.
// rec_out (optional, int64 [B]) receives i; cat == nullptr writes only rec_out.
//
// Hash of slot s, raw value c, V = vocab_per_slot in [1, 2³¹] (data.hash_rows):
//   salt = (s + 1)·0x9E3779B9 mod 2³²;  h = fmix32(c ^ salt)  (murmur3's finaliser)
//   ids[j][s] = s·V + ((h·V) >> 32)     64-bit: h·V < 2⁶³ and s·V ≤ S·V
// Dense (data.dense_norm): +0.0 if the stored value is INT_MIN, otherwise
//   fl(fl(float(v) − min[k]) / diff[k]): the int → fp32 conversion rounds to nearest
//   even, the subtraction and the division are each rounded once (the IEEE division,
//   as ctr.hip's Adagrad), so numpy's float32 has the same bits.
//
// One wave per row, four rows per 256-thread workgroup (ctr_fwd_kernel's shape); the
// S + n_dense + 1 columns of a row are taken by lane in steps of 64, so a wave reads
// and writes consecutive addresses.  The row index — and with it the Philox call and
// the 64-bit mod n — is wave-uniform.  Every read is of record src < n (staged:
// src = j < B) and happens only on a live row; column offsets stay below the row's width.
#include "common.h"
#include "kernels.h"

namespace pdo {

namespace {

// the drawn record of global row g; ≥ n only on the evaluation stream
__device__ __forceinline__ unsigned long long click_record(const DataDraw& d, unsigned long long g, unsigned long long n,
                                                           unsigned long long Bglobal) {
  if (d.stream != 0) return (unsigned long long)d.step * Bglobal + g;  // < 2³²·2³¹ + 2³²
  const Philox4 p = philox4x32_10((uint32_t)g, 0u, d.stream, d.step, d.key0, d.key1);
  return ((((unsigned long long)p.w[1] << 32) | p.w[0]) % n);
}

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__global__ __launch_bounds__(256) void click_records_kernel(long long n, int B, DataDraw d, unsigned long long Bglobal,
                                                            int64_t* __restrict__ rec_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= B) return;
  const unsigned long long i = click_record(d, d.row0 + (unsigned long long)j, (unsigned long long)n, Bglobal);
  rec_out[j] = i < (unsigned long long)n ? (int64_t)i : (int64_t)-1;
}

template <bool STAGED>
__global__ __launch_bounds__(256) void click_batch_kernel(const uint32_t* __restrict__ cat, const int* __restrict__ dense,
                                                          const uint8_t* __restrict__ label,
                                                          const float* __restrict__ stats, long long n, int B, int S,
                                                          int n_dense, unsigned long long V, int64_t* __restrict__ ids,
                                                          float* __restrict__ dense_out, float* __restrict__ label_out,
                                                          DataDraw d, unsigned long long Bglobal,
                                                          int64_t* __restrict__ rec_out) {
  const int j = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int lane = threadIdx.x & 63;
  if (j >= B) return;  // wave-uniform
  const unsigned long long i = click_record(d, d.row0 + (unsigned long long)j, (unsigned long long)n, Bglobal);
  const bool live = i < (unsigned long long)n;
  const size_t src = STAGED ? (size_t)j : (size_t)i;  // read on live rows only: src < n (staged: < B)
  if (lane == 0 && rec_out != nullptr) rec_out[j] = live ? (int64_t)i : (int64_t)-1;
  const int cols = S + n_dense + 1;
  for (int c = lane; c < cols; c += 64) {
    if (c < S) {
      int64_t id = -1;
      if (live) {
        const uint32_t h = fmix32(cat[src * S + c] ^ ((uint32_t)(c + 1) * 0x9E3779B9u));
        id = (int64_t)((unsigned long long)c * V + (((unsigned long long)h * V) >> 32));
      }
      ids[(size_t)j * S + c] = id;
    } else if (c < S + n_dense) {
      const int k = c - S;
      float x = 0.f;
      if (live) {
        const int v = dense[src * n_dense + k];
        if (v != INT_MIN) x = ((float)v - stats[k]) / stats[n_dense + k];
      }
      dense_out[(size_t)j * n_dense + k] = x;
    } else {
      label_out[j] = live ? (float)label[src] : -1.f;
    }
  }
}

}  // namespace

int click_batch(const uint32_t* cat, const int* dense, const uint8_t* label, const float* stats, long long n, int B,
                int S, int n_dense, long long V, int64_t* ids, float* dense_out, float* label_out, const DataDraw& draw,
                long long Bglobal, bool staged, int64_t* rec_out, hipStream_t st) {
  if (B < 1 || S < 1 || n_dense < 1 || (long long)B * S > INT_MAX || (long long)B * n_dense > INT_MAX) return -2;
  if (n < 1 || n > (1ll << 31) - 1 || Bglobal < B || Bglobal > (1ll << 31) || V < 1 || V > (1ll << 31)) return -3;
  if (draw.stream > 1 || draw.row0 + (unsigned long long)B > (1ull << 32)) return -4;  // g < 2^32
  if (cat == nullptr) {  // records only
    if (rec_out == nullptr) return -5;
    click_records_kernel<<<(B + 255) / 256, 256, 0, st>>>(n, B, draw, (unsigned long long)Bglobal, rec_out);
    return 0;
  }
  if (dense == nullptr || label == nullptr || stats == nullptr || ids == nullptr || dense_out == nullptr ||
      label_out == nullptr)
    return -5;
  const unsigned grid = (unsigned)((B + 3) / 4);
  if (staged)
    click_batch_kernel<true><<<grid, 256, 0, st>>>(cat, dense, label, stats, n, B, S, n_dense, (unsigned long long)V, ids,
                                                   dense_out, label_out, draw, (unsigned long long)Bglobal, rec_out);
  else
    click_batch_kernel<false><<<grid, 256, 0, st>>>(cat, dense, label, stats, n, B, S, n_dense, (unsigned long long)V,
                                                    ids, dense_out, label_out, draw, (unsigned long long)Bglobal, rec_out);
  return 0;
}

}  // namespace pdo
