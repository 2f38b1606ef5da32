// SPDX-License-Identifier: Apache-2.0
// Token batches from a uint16 corpus (gfx950): the window sampler of
// paddle_operator_amd/data.py and the uint16 → int64 widening, one launch.
//
// Row j of micro-batch m is the window tokens[start : start + S + 1]; idx is its
// first S tokens and tgt its last S.  With a draw, start comes from ONE
// Philox4x32-10 call (philox.h) per row: counter = (g, 0, stream, m) with
// g = row0 + j the global row (row0 = rank·B), key = (low, high) words of the data
// seed, start = ((w1 << 32) | w0) mod (n − S).  The host reference is
// paddle_operator_amd.data.window_starts.  Without a draw, tok is a staged
// [B][S + 1] buffer (the windows gathered on the host) and row j starts at j·(S + 1).
//
// A token ≥ vocab writes idx = 0 / tgt = −1 (embed_fwd stays inside its table,
// the cross-entropy skips the position) and adds 1 to *bad; every one of the
// B·(S + 1) window tokens is counted once.
//
// One token per lane: a window starts at any 2-byte offset, so a lane loads one
// uint16 (a wave reads 128 contiguous bytes) and stores 8 B to idx and to tgt.
// The largest address read is tok[start + S] ≤ tok[n − 1].  The traffic is the
// 16 B written per token (0.5 MB at B = 32, S = 1024): the launch, not the access
// width, is the cost of this kernel.
#include "common.h"
#include "kernels.h"

namespace pdo {

__device__ __forceinline__ long long window_start(const DataDraw& d, unsigned long long g, long long span) {
  const Philox4 p = philox4x32_10((uint32_t)g, 0u, d.stream, d.step, d.key0, d.key1);
  const unsigned long long r = ((unsigned long long)p.w[1] << 32) | p.w[0];
  return (long long)(r % (unsigned long long)span);
}

template <bool DRAW>
__global__ __launch_bounds__(256) void token_batch_kernel(const uint16_t* __restrict__ tok, long long n, int S,
                                                          int vocab, int64_t* __restrict__ idx,
                                                          int64_t* __restrict__ tgt,
                                                          unsigned long long* __restrict__ bad, DataDraw d,
                                                          int64_t* __restrict__ starts_out) {
  const int j = blockIdx.y;
  const long long start = DRAW ? window_start(d, d.row0 + (unsigned long long)j, n - S) : (long long)j * (S + 1);
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (DRAW && starts_out != nullptr && t == 0) starts_out[j] = start;
  if (t > S) return;
  const int v = tok[start + t];
  const bool ok = v < vocab;
  if (t < S) idx[(long long)j * S + t] = ok ? v : 0;
  if (t > 0) tgt[(long long)j * S + t - 1] = ok ? v : -1;
  if (!ok) atomicAdd(bad, 1ull);
}

__global__ __launch_bounds__(256) void window_starts_kernel(long long n, int B, int S, DataDraw d,
                                                            int64_t* __restrict__ starts_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < B) starts_out[j] = window_start(d, d.row0 + (unsigned long long)j, n - S);
}

int token_batch(const uint16_t* tok, long long n, int B, int S, int vocab, int64_t* idx, int64_t* tgt,
                unsigned long long* bad, const DataDraw* draw, int64_t* starts_out, hipStream_t st) {
  if (B < 1 || S < 1 || vocab < 1 || vocab > 65536) return -2;
  if (draw != nullptr) {
    if (n < (long long)S + 1) return -3;
    if (draw->row0 + (unsigned long long)B > (1ull << 32)) return -4;  // g < 2^32
  } else if (tok == nullptr || n != (long long)B * (S + 1)) {
    return -3;
  }
  if (tok == nullptr) {  // starts only
    if (starts_out == nullptr) return -5;
    window_starts_kernel<<<(B + 255) / 256, 256, 0, st>>>(n, B, S, *draw, starts_out);
    return 0;
  }
  if (idx == nullptr || tgt == nullptr || bad == nullptr || B > 65535) return -5;
  const dim3 grid((unsigned)(S / 256 + 1), (unsigned)B);  // S + 1 tokens per row
  if (draw != nullptr) token_batch_kernel<true><<<grid, 256, 0, st>>>(tok, n, S, vocab, idx, tgt, bad, *draw, starts_out);
  else token_batch_kernel<false><<<grid, 256, 0, st>>>(tok, n, S, vocab, idx, tgt, bad, DataDraw{}, nullptr);
  return 0;
}

}  // namespace pdo
