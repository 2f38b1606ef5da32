// SPDX-License-Identifier: Apache-2.0
// LayerNorm forward/backward (optionally fused with the residual add) for
// gfx950.  One wave per row: a row of C bf16 is held in registers as VPL
// vectors of 8 (16-B loads), statistics are two-pass in registers (exact
// mean, then centred variance), reductions are 64-lane shuffles.  Backward
// computes dx per row and accumulates dgamma/dbeta per lane in registers over
// a grid-stride row loop; the 4 waves of a block combine through LDS and the
// per-block partials are summed by the two-level `colsum` (reduce.hip).
//
// DROP instantiations: dropout of the residual branch, h = x + drop(r + rbias),
// from the counter-based mask of philox.h — one Philox call per 16-B vector in
// the forward, the same call again in the backward, no stored mask.  The
// DROP = false instantiations are the kernels as they were (the DropArgs
// argument is last and unread).
#include "common.h"
#include "kernels.h"

namespace pdo {

// v scaled where bit j of keep is set, +0 elsewhere
__device__ __forceinline__ f32x8 drop_apply(f32x8 v, uint32_t keep, float scale) {
  f32x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (keep >> j) & 1u ? v[j] * scale : 0.f;
  return o;
}

template <int VPL, bool ADD, bool DROP = false>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ r,
                                                     const bf16* __restrict__ rb,
                                                     const bf16* __restrict__ w, const bf16* __restrict__ b,
                                                     bf16* __restrict__ h, bf16* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     int N, int C, float eps, DropArgs drop) {
  static_assert(ADD || !DROP, "dropout applies to the residual branch");
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;
  const size_t base = (size_t)row * C;
  const bf16x8* xr = reinterpret_cast<const bf16x8*>(x + base);
  const bf16x8* rr = reinterpret_cast<const bf16x8*>(r + base);
  const int C8 = C >> 3;
  f32x8 v[VPL];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c8 = lane + i * 64;
    if (c8 < C8) {
      v[i] = to_f32(xr[c8]);
      if (ADD && !DROP) {
        v[i] += to_f32(rr[c8]);
        if (rb) v[i] += to_f32(reinterpret_cast<const bf16x8*>(rb)[c8]);
      }
      if (DROP) {
        f32x8 t = to_f32(rr[c8]);
        if (rb) t += to_f32(reinterpret_cast<const bf16x8*>(rb)[c8]);
        v[i] += drop_apply(t, drop_keep_bits(drop, (uint64_t)row * C8 + c8), drop.scale);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[i][j];
    } else {
      v[i] = f32x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const float inv_c = 1.f / (float)C;
  const float mean = wave_sum(s) * inv_c;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c8 = lane + i * 64;
    if (c8 < C8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = v[i][j] - mean;
        q += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) * inv_c + eps);
  const bf16x8* wr = reinterpret_cast<const bf16x8*>(w);
  const bf16x8* br = reinterpret_cast<const bf16x8*>(b);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c8 = lane + i * 64;
    if (c8 < C8) {
      if (ADD) reinterpret_cast<bf16x8*>(h + base)[c8] = to_bf16(v[i]);
      f32x8 wf = to_f32(wr[c8]), bf = to_f32(br[c8]);
      f32x8 o = (v[i] - mean) * rstd * wf + bf;
      reinterpret_cast<bf16x8*>(y + base)[c8] = to_bf16(o);
    }
  }
  if (lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
}

// NA = 2: partials (dgamma, dbeta); NA = 3: + colsum(dx) — the gradient of a
// bias folded into the residual branch (h = x + r + rbias).
// DROP: `ddrop` = keep ? o·scale : 0 beside dx = o (dx may be null), and the
// NA = 3 accumulator sums the masked, scaled value (the bias sits inside the dropout).
template <int VPL, bool ADD, int NA, bool DROP = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                     const bf16* __restrict__ w, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const bf16* __restrict__ dres,
                                                     bf16* __restrict__ dx, float* __restrict__ part, int N, int C,
                                                     bf16* __restrict__ ddrop, DropArgs drop) {
  static_assert(ADD || !DROP, "dropout applies to the residual branch");
  constexpr int COLS = 64 * 8 * VPL;
  __shared__ float red[NA * COLS];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int C8 = C >> 3;
  const float inv_c = 1.f / (float)C;
  f32x8 wv[VPL], adw[VPL], adb[VPL], adx[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c8 = lane + i * 64;
    wv[i] = c8 < C8 ? to_f32(reinterpret_cast<const bf16x8*>(w)[c8]) : f32x8{0, 0, 0, 0, 0, 0, 0, 0};
    adw[i] = f32x8{0, 0, 0, 0, 0, 0, 0, 0};
    adb[i] = adw[i];
    adx[i] = adw[i];
  }
  const int nw = gridDim.x * 4;
  // every operand of a row (dy, x and the residual gradient) is requested
  // up front, and the NEXT row's are requested before this row's two
  // wave-wide reductions: the reductions' latency hides the loads'
  bf16x8 nd[VPL], nx[VPL], nr[VPL];
  auto fetch = [&](int row) {
    const size_t base = (size_t)row * C;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c8 = lane + i * 64;
      if (c8 < C8) {
        nd[i] = reinterpret_cast<const bf16x8*>(dy + base)[c8];
        nx[i] = reinterpret_cast<const bf16x8*>(x + base)[c8];
        if (ADD) nr[i] = reinterpret_cast<const bf16x8*>(dres + base)[c8];
      }
    }
  };
  int row = blockIdx.x * 4 + wid;
  if (row < N) fetch(row);
  for (; row < N; row += nw) {
    const size_t base = (size_t)row * C;
    const float mu = mean[row], rs = rstd[row];
    f32x8 xh[VPL], g[VPL], rr[VPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c8 = lane + i * 64;
      if (c8 < C8) {
        f32x8 d = to_f32(nd[i]);
        f32x8 xv = to_f32(nx[i]);
        if (ADD) rr[i] = to_f32(nr[i]);
        xh[i] = (xv - mu) * rs;
        g[i] = d * wv[i];
        adw[i] += d * xh[i];
        adb[i] += d;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s1 += g[i][j];
          s2 += g[i][j] * xh[i][j];
        }
      }
    }
    if (row + nw < N) fetch(row + nw);
    s1 = wave_sum(s1) * inv_c;
    s2 = wave_sum(s2) * inv_c;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c8 = lane + i * 64;
      if (c8 < C8) {
        f32x8 o = (g[i] - s1 - xh[i] * s2) * rs;
        if (ADD) o += rr[i];
        if (DROP) {
          // the bias gradient sums ddrop as stored (rounded to bf16): it is the column
          // sum of the very gradient the branch GEMM's backward reads, as bias_grad
          // over that tensor would give
          const bf16x8 od = to_bf16(drop_apply(o, drop_keep_bits(drop, (uint64_t)row * C8 + c8), drop.scale));
          if (NA == 3) adx[i] += to_f32(od);
          reinterpret_cast<bf16x8*>(ddrop + base)[c8] = od;
          if (dx) reinterpret_cast<bf16x8*>(dx + base)[c8] = to_bf16(o);
        } else {
          if (NA == 3) adx[i] += o;
          reinterpret_cast<bf16x8*>(dx + base)[c8] = to_bf16(o);
        }
      }
    }
  }
  // combine the 4 waves sequentially through one [NA][COLS] LDS image
  for (int k = 0; k < 4; ++k) {
    if (wid == k) {
#pragma unroll
      for (int i = 0; i < VPL; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = (i * 64 + lane) * 8 + j;
          const float a0 = adw[i][j], a1 = adb[i][j], a2 = adx[i][j];
          if (k == 0) {
            red[c] = a0;
            red[COLS + c] = a1;
            if (NA == 3) red[2 * COLS + c] = a2;
          } else {
            red[c] += a0;
            red[COLS + c] += a1;
            if (NA == 3) red[2 * COLS + c] += a2;
          }
        }
    }
    __syncthreads();
  }
  float* pp = part + (size_t)blockIdx.x * NA * C;
  for (int k = threadIdx.x; k < NA * C; k += 256) {
    const int a = k / C, c = k - a * C;
    pp[k] = red[a * COLS + c];
  }
}

#define LN_DISPATCH(VPL_, ...)                  \
  switch (VPL_) {                               \
    case 1: { constexpr int V = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int V = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int V = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int V = 4; __VA_ARGS__; } break; \
    case 5: { constexpr int V = 5; __VA_ARGS__; } break; \
    case 6: { constexpr int V = 6; __VA_ARGS__; } break; \
    case 8: { constexpr int V = 8; __VA_ARGS__; } break; \
    default: return -1;                         \
  }

static int vpl_for(int C) {
  int v = (C + 511) / 512;
  if (v == 7) v = 8;
  return v;
}

int layernorm_fwd(const bf16* x, const bf16* r, const bf16* rb, const bf16* w, const bf16* b, bf16* h, bf16* y,
                  float* mean, float* rstd, int N, int C, float eps, hipStream_t st, const DropArgs* drop) {
  if (C % 8 != 0 || C > 4096) return -2;
  if (rb && !r) return -4;
  if (drop && (drop->thr > 65535u || (drop->thr && !r))) return -6;
  const int grid = (N + 3) / 4;
  const int vpl = vpl_for(C);
  const DropArgs d = drop ? *drop : DropArgs();
  if (d.thr) {
    LN_DISPATCH(vpl, ln_fwd_kernel<V, true, true><<<grid, 256, 0, st>>>(x, r, rb, w, b, h, y, mean, rstd, N, C, eps, d))
  } else if (r) {
    LN_DISPATCH(vpl, ln_fwd_kernel<V, true><<<grid, 256, 0, st>>>(x, r, rb, w, b, h, y, mean, rstd, N, C, eps, d))
  } else {
    LN_DISPATCH(vpl, ln_fwd_kernel<V, false><<<grid, 256, 0, st>>>(x, r, rb, w, b, h, y, mean, rstd, N, C, eps, d))
  }
  return 0;
}

int layernorm_bwd_grid(int N) {
  // one resident round: ≤ 2 waves/SIMD at this kernel's register count
  // (4 waves per block, 256 CUs × 4 SIMDs × 2 / 4 = 512 blocks), ≥ 4 rows per wave
  int g = (N + 15) / 16;
  if (g > 512) g = 512;
  if (g < 1) g = 1;
  return g;
}

// out: dgamma | dbeta | (drbias) as C-column segments; part: [grid][NA*C] f32;
// scratch: colsum_scratch_floats(grid, NA*C)
int layernorm_bwd(const bf16* dy, const bf16* x, const bf16* w, const float* mean, const float* rstd,
                  const bf16* dres, bf16* dx, float* part, float* scratch, const ColOut& out, bool rbias, int N,
                  int C, hipStream_t st, bool reduce, const DropArgs* drop, bf16* ddrop) {
  if (C % 8 != 0 || C > 4096) return -2;
  if (rbias && !dres) return -4;
  if (out.seg != C) return -5;
  if (drop && (drop->thr > 65535u || (drop->thr && (!dres || !ddrop)))) return -6;
  const DropArgs d = drop ? *drop : DropArgs();
  if (!d.thr && !dx) return -7;  // only the DROP kernels take a null dx
  const int grid = layernorm_bwd_grid(N);
  const int vpl = vpl_for(C);
  if (vpl > 4) return -3;  // register/LDS budget of the in-block combine
  const int NA = rbias ? 3 : 2;
#define LN_BWD(ADD_, NA_, DROP_) \
  LN_DISPATCH(vpl, ln_bwd_kernel<V, ADD_, NA_, DROP_><<<grid, 256, 0, st>>>(dy, x, w, mean, rstd, dres, dx, part, N, C, ddrop, d))
  if (d.thr && rbias) {
    LN_BWD(true, 3, true)
  } else if (d.thr) {
    LN_BWD(true, 2, true)
  } else if (rbias) {
    LN_BWD(true, 3, false)
  } else if (dres) {
    LN_BWD(true, 2, false)
  } else {
    LN_BWD(false, 2, false)
  }
#undef LN_BWD
  if (reduce) colsum(part, grid, NA * C, NA * C, out, scratch, st);
  return 0;
}

}  // namespace pdo
