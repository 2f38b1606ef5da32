// SPDX-License-Identifier: Apache-2.0
// LARS (layer-wise adaptive rate scaling, Paddle's lars_momentum) over the flat
// fp32 arena of ResNet-50 (workloads/resnet.py FlatLARS), gfx950.
//
//   g  = grad_scale · grad
//   λ_t = coeff · ‖w_t‖ / (‖g_t‖ + wd·‖w_t‖ + eps)   for a decayed tensor with ‖w_t‖ > 0 and ‖g_t‖ > 0,
//   λ_t = 1                                            otherwise
//   v ← mom·v + (lr·λ_t)·(g + (wd·dec)·w),   w ← w − v
//
// Three launches on one stream, no atomics, no waiting between workgroups; every
// tensor of the arena starts on a 1,024-element chunk boundary and its padding is zero,
// so a tensor's norm is the norm of its chunks.
//
// Summation order (fixed: two runs on the same inputs are bitwise equal).  For Σw² and
// Σg² alike, with K the tensor's chunk count:
//   pass A, per lane:     lane l of the chunk's wave holds the f32x4 vectors l, l + 64,
//                         l + 128, l + 192 of the chunk and adds their 16 squares in
//                         memory order into one accumulator that starts at 0 — 16 additions;
//   pass A, across lanes: the xor butterfly of wave_sum, offsets 32, 16, …, 1 — 6 additions;
//   pass B, per lane:     thread t of the tensor's 256-thread workgroup adds the chunk
//                         partials t, t + 256, t + 512, … in that order into an accumulator
//                         that starts at 0 — ceil(K / 256) additions;
//   pass B, across lanes: the same butterfly inside each of the 4 waves — 6 additions;
//   pass B, across waves: wave 0 + wave 1 + wave 2 + wave 3, left to right — 3 additions.
// Longest path: 16 + 6 + ceil(K / 256) + 6 + 3 = 31 + ceil(K / 256) additions (40 for
// ResNet-50's largest tensor, 2,304 chunks).  The square roots, the product wd·‖w‖, the
// two additions of the denominator, coeff·‖w‖ and the division are IEEE fp32, one rounding each.
//
// Pass A runs one wave per chunk, four chunks per 256-thread workgroup, grid-stride:
// a chunk is 4 KiB = 64 lanes × 4 × 16 B, so a wave issues its 8 loads (w and g) at once
// and reduces with shuffles alone — no LDS, no barrier, and a quarter of the workgroups
// of a block-per-chunk launch (ResNet-50: 24,978 chunks on 2,048 resident workgroups,
// about three chunks per wave).  Pass B is one workgroup per tensor: at most 9 loads per
// thread for 2,304 chunks, then the tree above.  Pass C is sgd_kernel's stream with one
// more float per chunk (ratio_chunks, written by pass B).
//
// This file is compiled without packed fp32 instructions (tools/build.py hip_flags).
#include "common.h"
#include "kernels.h"

namespace pdo {

// part[2c] = Σ w², part[2c + 1] = Σ (grad_scale·g)² over chunk c
__global__ __launch_bounds__(256) void lars_partial_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                           int chunks, float grad_scale, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < chunks; c += gridDim.x * 4) {
    const f32x4* wp = reinterpret_cast<const f32x4*>(w) + (long long)c * 256 + lane;
    const f32x4* gp = reinterpret_cast<const f32x4*>(g) + (long long)c * 256 + lane;
    f32x4 wv[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      wv[u] = wp[64 * u];
      gv[u] = gp[64 * u];
    }
    float sw = 0.f, sg = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gj = gv[u][j] * grad_scale;
        sw += wv[u][j] * wv[u][j];
        sg += gj * gj;
      }
    }
    sw = wave_sum(sw);
    sg = wave_sum(sg);
    if (lane == 0) {
      part[2 * c] = sw;
      part[2 * c + 1] = sg;
    }
  }
}

// one workgroup per tensor: table[3t..3t+3) = (first chunk, chunk count, decay flag);
// ratio_chunks[c] = λ_t for every chunk of the tensor
__global__ __launch_bounds__(256) void lars_ratio_kernel(const float* __restrict__ part,
                                                         const int* __restrict__ table, int chunks, float coeff,
                                                         float eps, float wd, float* __restrict__ ratio_chunks) {
  __shared__ float red[8];
  const int c0 = table[3 * blockIdx.x], K = table[3 * blockIdx.x + 1], decayed = table[3 * blockIdx.x + 2];
  if (c0 < 0 || K < 1 || K > chunks - c0) return;  // a device table that is not the checked host table
  float lam = 1.f;
  if (decayed) {  // uniform over the workgroup
    float sw = 0.f, sg = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
      sw += part[2 * (c0 + k)];
      sg += part[2 * (c0 + k) + 1];
    }
    sw = wave_sum(sw);
    sg = wave_sum(sg);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      red[wv] = sw;
      red[4 + wv] = sg;
    }
    __syncthreads();
    sw = ((red[0] + red[1]) + red[2]) + red[3];
    sg = ((red[4] + red[5]) + red[6]) + red[7];
    const float W = sqrtf(sw), G = sqrtf(sg);
    if (W > 0.f && G > 0.f) lam = (coeff * W) / ((G + wd * W) + eps);
  }
  for (int k = threadIdx.x; k < K; k += 256) ratio_chunks[c0 + k] = lam;
}

// the rate by value or, lr_dev given, from device memory (a schedule under a captured
// step): one kernel for both, so the two results are the same bits
__global__ __launch_bounds__(256) void lars_update_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                          float* __restrict__ buf,
                                                          const float* __restrict__ decay_chunks,
                                                          const float* __restrict__ ratio_chunks, long long n4,
                                                          float lr_val, const float* __restrict__ lr_dev, float mom,
                                                          float wd, float grad_scale) {
  const float lr = lr_dev ? *lr_dev : lr_val;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float dec = decay_chunks[i >> 8];  // 1024 elements per chunk = 256 f32x4
    const float rate = lr * ratio_chunks[i >> 8];
    const f32x4 gi = reinterpret_cast<const f32x4*>(g)[i] * grad_scale;
    f32x4 wi = reinterpret_cast<const f32x4*>(w)[i];
    f32x4 b = reinterpret_cast<const f32x4*>(buf)[i];
    b = mom * b + rate * (gi + (wd * dec) * wi);
    wi = wi - b;
    reinterpret_cast<f32x4*>(buf)[i] = b;
    reinterpret_cast<f32x4*>(w)[i] = wi;
  }
}

int lars_flat(float* w, const float* g, float* buf, const float* decay_chunks, float* ratio_chunks, float* part,
              const int* table, const int* table_host, int tensors, long long n, float lr, float mom, float wd,
              float coeff, float eps, float grad_scale, hipStream_t st, const float* lr_dev) {
  if (n <= 0 || n % 1024 || n / 1024 > 0x3fffffff) return -2;
  const int chunks = (int)(n / 1024);
  if (tensors < 1 || tensors > chunks) return -3;
  int want = 0;  // the tensors tile the arena's chunks in order, without gaps
  for (int t = 0; t < tensors; ++t) {
    const int c0 = table_host[3 * t], K = table_host[3 * t + 1], dec = table_host[3 * t + 2];
    if (c0 != want || K < 1 || K > chunks - c0 || (dec != 0 && dec != 1)) return -3;
    want = c0 + K;
  }
  if (want != chunks) return -3;
  lars_partial_kernel<<<stream_grid(chunks, 4), 256, 0, st>>>(w, g, chunks, grad_scale, part);
  lars_ratio_kernel<<<tensors, 256, 0, st>>>(part, table, chunks, coeff, eps, wd, ratio_chunks);
  lars_update_kernel<<<stream_grid(n / 4, 256), 256, 0, st>>>(w, g, buf, decay_chunks, ratio_chunks, n / 4, lr, lr_dev,
                                                             mom, wd, grad_scale);
  return 0;
}

}  // namespace pdo
