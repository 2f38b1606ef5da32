// SPDX-License-Identifier: Apache-2.0
// Sparse side of the CTR models (Wide&Deep, DeepFM) on gfx950: the fused lookup
// of a batch and the deterministic sparse backward with its row-wise Adagrad.
//
// Tables are fp32: deep[rows, D], wide[rows], accumulators of the same shapes;
// ids are int64.  Flat lookup i of N = B·S belongs to sample i / S, slot i % S.
// Contract: D % 4 == 0 and 4 <= D <= 64 (L = D/4 lanes of 16 B hold one row);
// anything else is refused with -2 before a launch.  An id outside [0, rows)
// reads nothing: zeros in the forward, no contribution in the backward (the
// rule of embed.hip).  Every index is checked before it is used.
//
// ---- ctr_fwd: one wave per sample, one launch per batch --------------------
// Lane l of the wave is (r, c) = (l / L, l % L) with R = 64 / L rows side by
// side (lanes >= R·L idle); pass p = 0 … P-1 (P = ceil(S / R)) serves slot
// p·R + r: one 16-B load of deep[id, 4c : 4c+4], one 16-B store into
// X[b, slot·D + 4c] (four 4-B stores when ldx % 4 != 0) — at D = 16 a wave
// instruction moves 16 rows = 1 KiB.  The dense features are copied to
// X[b, S·D : S·D + n_dense] and the padding columns X[b, S·D + n_dense : ldx]
// are written as zeros.
//
// Sums, in this fixed order (V = min(R, S) lanes of a column hold values):
//   * per lane over its passes, p ascending:     w += wide[id];  s += e;
//     q = fma(e, e, q)                            (P − 1 additions; the first
//     pass adds to zero, which is exact; q takes one rounding per pass)
//   * over r by a tree, distance 32, 16, …, 1 rows: lane (r, c), r < dist, adds
//     the value of lane (r + dist, c) when r + dist < R   (ceil(log2 V)
//     roundings, the rest adds zeros)
//   wide_sum[b] = w of lane (0, 0);  ssum[b, 4c : 4c+4] = s of lane (0, c).
//   fm: lane (0, c): t = Σ_j (s_j·s_j − q_j), j = 0 … 3 ascending, each term
//   fma(s_j, s_j, −q_j); then a tree over c, distance 8, 4, 2, 1 lanes (lane
//   c < dist adds lane c + dist when c + dist < L); fm[b] = 0.5·t (exact).
// fp32 roundings on the longest path, CS = (P − 1) + ceil(log2 V):
//   wide_sum, ssum:  CS
//   fm:              2·CS + 1 (s_j² with both factors carrying CS, fused with
//                    the subtraction) + 3 (sum over j) + ceil(log2 L)
// relative to Σ|terms|, where fm's terms are those of the expanded form
// ½ Σ_d (Σ_{i,j} e_i·e_j − Σ_i e_i²).
//
// ---- ctr_bwd_rows: segmented sum over the stably sorted ids ----------------
// keys / perm = the lookups' ids sorted stably and their flat indices.  A group
// of G lanes (G = 4, 8 or 16, the smallest holding L) owns one sorted position;
// the group at the first position of a PIECE — a run of equal keys cut at
// CTR_SEG-position segment boundaries — sums the piece in sorted order, k
// ascending, with b = perm[k] / S, slot = perm[k] % S:
//   a  += dX[b, slot·D + d]                       (every mode)
//   t   = fma(dlogit[b], ssum[b, d], t)           (fm only)
//   sd += dlogit[b]                               (= the wide gradient)
// A run inside one segment is finished by its group; the pieces of a run that
// crosses a boundary leave (a, t, sd) in `part` (segment s: [first piece |
// last piece] × (2·D + 4) floats) and ctr_bwd_fold_kernel adds them in segment
// order, each of a, t, sd on its own.  Then, e being the table row (the same
// for the whole run, read before it is written by the one group that owns it):
//   g[d] = fma(−e[d], sd, a[d] + t[d])  (fm)      g[d] = a[d]  (no fm)
//   g_w  = sd
// No atomics, no dense gradient table, no per-lookup gradient array; the result
// does not depend on scheduling.  Rows whose id is not in the batch are neither
// read nor written.
// Roundings of g for a run of n lookups, relative to Σ|terms|: at most n − 1
// without fm (a; the first addition is to zero) and n + 2 with fm (t: n fused
// multiply-adds, then a + t and the final fma); g_w: n − 1.
//
// GRAD:    g_deep[key, :] = g, g_wide[key] = g_w (overwritten, not accumulated).
// ADAGRAD: per element, with lr loaded from a device float
//   acc' = fma(g, g, acc)                         1 rounding
//   w'   = w − (lr·g) / sqrt(acc')                lr·g: 1, sqrt: 1, division: 1,
//                                                 subtraction: 1
// sqrt and the division are the IEEE correctly rounded ones (the compiler's
// default for HIP), not the hardware approximations optim.hip's AdamW uses:
// this touches only the batch's rows, the longer sequences cost nothing that
// shows.  With g carrying CG roundings, acc' is within half an ulp of its exact
// value plus (2·CG + 1)·2⁻²⁴·g², and w' within half an ulp plus
// (2·CG + 4)·2⁻²⁴·|lr·g / sqrt(acc')| (g: CG, lr·g: 1, sqrt of acc': CG + 1.5,
// division: 1, rounded up).
#include "common.h"
#include "kernels.h"

namespace pdo {

constexpr int CTR_SEG = 256;  // sorted positions per segment of the sparse backward

__device__ __forceinline__ f32x4 ctr_load4(const float* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}

__device__ __forceinline__ void ctr_store4(float* p, f32x4 v, bool aligned) {
  if (aligned) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    p[0] = v[0];
    p[1] = v[1];
    p[2] = v[2];
    p[3] = v[3];
  }
}

template <bool FM>
__global__ __launch_bounds__(256) void ctr_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dense,
                                                      const float* __restrict__ deep, const float* __restrict__ wide,
                                                      float* __restrict__ X, float* __restrict__ wide_sum,
                                                      float* __restrict__ ssum, float* __restrict__ fm, int B, int S,
                                                      int D, int n_dense, int ldx, long long rows) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;  // wave-uniform: the shuffles below run with all 64 lanes
  const int L = D >> 2, R = 64 / L;
  const int r = lane / L, c = lane - r * L;
  const bool live = r < R;
  const bool al = (ldx & 3) == 0;
  float* xrow = X + (size_t)b * ldx;
  f32x4 s = {0, 0, 0, 0}, q = {0, 0, 0, 0};
  float w = 0.f;
  for (int s0 = 0; s0 < S; s0 += R) {
    const int slot = s0 + r;
    if (!live || slot >= S) continue;
    const int64_t id = ids[(size_t)b * S + slot];
    f32x4 e = {0, 0, 0, 0};
    if (id >= 0 && id < rows) {
      e = *reinterpret_cast<const f32x4*>(deep + (size_t)id * D + 4 * c);
      if (c == 0) w += wide[id];
    }
    ctr_store4(xrow + (size_t)slot * D + 4 * c, e, al);
    s += e;
    if (FM) {
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = __builtin_fmaf(e[j], e[j], q[j]);
    }
  }
  const int SD = S * D;
  for (int k = lane; k < n_dense; k += 64) xrow[SD + k] = dense[(size_t)b * n_dense + k];
  for (int k = SD + n_dense + lane; k < ldx; k += 64) xrow[k] = 0.f;
  // tree over r: lane (r, c) += lane (r + dist, c)
#pragma unroll
  for (int dist = 32; dist > 0; dist >>= 1) {
    const int src = lane + dist * L;
    const bool ok = live && r < dist && r + dist < R;  // then src < R·L <= 64
    const int from = ok ? src : lane;
    const float w2 = __shfl(w, from, 64);
    w += ok ? w2 : 0.f;
    if (FM) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s2 = __shfl(s[j], from, 64), q2 = __shfl(q[j], from, 64);
        s[j] += ok ? s2 : 0.f;
        q[j] += ok ? q2 : 0.f;
      }
    }
  }
  if (lane == 0) wide_sum[b] = w;
  if (FM) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) t += __builtin_fmaf(s[j], s[j], -q[j]);
#pragma unroll
    for (int dist = 8; dist > 0; dist >>= 1) {
      const bool ok = lane < dist && lane + dist < L;
      const float t2 = __shfl(t, ok ? lane + dist : lane, 64);
      t += ok ? t2 : 0.f;
    }
    if (lane < L) *reinterpret_cast<f32x4*>(ssum + (size_t)b * D + 4 * lane) = s;
    if (lane == 0) fm[b] = 0.5f * t;
  }
}

struct CtrBwdArgs {
  const int64_t* keys;
  const int64_t* perm;
  const float* dX;
  const float* dlogit;
  const float* ssum;
  float* part;
  float* deep;      // table (read for fm; updated by ADAGRAD)
  float* wide;
  float* out_deep;  // GRAD: g_deep; ADAGRAD: the deep accumulator
  float* out_wide;  // GRAD: g_wide; ADAGRAD: the wide accumulator
  const float* lr;
  int N, S, D, ldx;
  long long rows;
};

// the run's sums are complete: write the gradient (GRAD) or apply Adagrad
template <bool FM, int MODE>
__device__ __forceinline__ void ctr_finish(const CtrBwdArgs& A, int64_t key, int c, f32x4 a, f32x4 t, float sd) {
  float* wrow = A.deep + (size_t)key * A.D + 4 * c;
  f32x4 g = a;
  if (FM) {
    const f32x4 e = *reinterpret_cast<const f32x4*>(wrow);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = __builtin_fmaf(-e[j], sd, a[j] + t[j]);
  }
  float* orow = A.out_deep + (size_t)key * A.D + 4 * c;
  if (MODE == CTR_GRAD) {
    *reinterpret_cast<f32x4*>(orow) = g;
    if (c == 0) A.out_wide[key] = sd;
    return;
  }
  const float lr = *A.lr;
  f32x4 acc = *reinterpret_cast<const f32x4*>(orow);
  f32x4 w = *reinterpret_cast<const f32x4*>(wrow);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = __builtin_fmaf(g[j], g[j], acc[j]);
    w[j] = w[j] - (lr * g[j]) / sqrtf(acc[j]);
  }
  *reinterpret_cast<f32x4*>(orow) = acc;
  *reinterpret_cast<f32x4*>(wrow) = w;
  if (c == 0) {
    const float aw = __builtin_fmaf(sd, sd, A.out_wide[key]);
    A.out_wide[key] = aw;
    A.wide[key] = A.wide[key] - (lr * sd) / sqrtf(aw);
  }
}

template <int G, bool FM, int MODE>
__global__ __launch_bounds__(256) void ctr_bwd_rows_kernel(CtrBwdArgs A) {
  const int i = blockIdx.x * (256 / G) + threadIdx.x / G;
  const int c = threadIdx.x % G;
  const int L = A.D >> 2, N = A.N;
  if (i >= N || c >= L) return;
  const int64_t key = A.keys[i];
  const bool cont = i > 0 && A.keys[i - 1] == key;  // continues a run from before
  if (cont && i % CTR_SEG != 0) return;             // not the start of a piece
  if (key < 0 || key >= A.rows) return;             // ids outside the table contribute nothing
  const int seg = i / CTR_SEG, seg_end = min(N, (seg + 1) * CTR_SEG);
  int j = i;
  while (j < seg_end && A.keys[j] == key) ++j;
  const bool more = j == seg_end && j < N && A.keys[j] == key;  // run goes on past the segment
  const bool al = (A.ldx & 3) == 0;
  f32x4 a = {0, 0, 0, 0}, t = {0, 0, 0, 0};
  float sd = 0.f;
  for (int k = i; k < j; ++k) {
    const int64_t p = A.perm[k];
    if (p < 0 || p >= N) continue;  // not a lookup of this batch
    const int b = (int)(p / A.S), slot = (int)(p - (int64_t)b * A.S);
    a += ctr_load4(A.dX + (size_t)b * A.ldx + (size_t)slot * A.D + 4 * c, al);
    const float dl = A.dlogit[b];
    sd += dl;
    if (FM) {
      const f32x4 ss = *reinterpret_cast<const f32x4*>(A.ssum + (size_t)b * A.D + 4 * c);
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = __builtin_fmaf(dl, ss[q], t[q]);
    }
  }
  if (!cont && !more) {
    ctr_finish<FM, MODE>(A, key, c, a, t, sd);
    return;
  }
  const int PW = 2 * A.D + 4;
  float* dst = A.part + ((size_t)seg * 2 + (cont ? 0 : 1)) * PW;
  *reinterpret_cast<f32x4*>(dst + 4 * c) = a;
  *reinterpret_cast<f32x4*>(dst + A.D + 4 * c) = t;
  if (c == 0) *reinterpret_cast<f32x4*>(dst + 2 * A.D) = f32x4{sd, 0.f, 0.f, 0.f};
}

// the runs that cross segment boundaries: the group of the run's start adds its
// last-piece partial and the following segments' first-piece partials, in order
template <int G, bool FM, int MODE>
__global__ __launch_bounds__(256) void ctr_bwd_fold_kernel(CtrBwdArgs A) {
  const int i = blockIdx.x * (256 / G) + threadIdx.x / G;
  const int c = threadIdx.x % G;
  const int L = A.D >> 2, N = A.N;
  if (i >= N || c >= L) return;
  const int64_t key = A.keys[i];
  if ((i > 0 && A.keys[i - 1] == key) || key < 0 || key >= A.rows) return;  // run starts only
  const int seg = i / CTR_SEG, seg_end = (seg + 1) * CTR_SEG;
  if (seg_end >= N || A.keys[seg_end] != key || A.keys[seg_end - 1] != key) return;  // no boundary crossed
  const int PW = 2 * A.D + 4;
  const float* p = A.part + ((size_t)seg * 2 + 1) * PW;
  f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * c);
  f32x4 t = *reinterpret_cast<const f32x4*>(p + A.D + 4 * c);
  float sd = p[2 * A.D];
  for (int s2 = seg + 1; s2 * CTR_SEG < N && A.keys[s2 * CTR_SEG] == key; ++s2) {
    const float* q = A.part + ((size_t)s2 * 2) * PW;
    a += *reinterpret_cast<const f32x4*>(q + 4 * c);
    t += *reinterpret_cast<const f32x4*>(q + A.D + 4 * c);
    sd += q[2 * A.D];
  }
  ctr_finish<FM, MODE>(A, key, c, a, t, sd);
}

static bool ctr_dim_ok(int D) { return D % 4 == 0 && D >= 4 && D <= 64; }

int ctr_fwd(const int64_t* ids, const float* dense, const float* deep, const float* wide, float* X, float* wide_sum,
            float* ssum, float* fm, int B, int S, int D, int n_dense, int ldx, long long rows, hipStream_t st) {
  if (!ctr_dim_ok(D)) return -2;
  if (B < 0 || S < 1 || n_dense < 0 || rows < 0 || (long long)S * D + n_dense > ldx) return -2;
  if ((fm == nullptr) != (ssum == nullptr)) return -2;
  if (B == 0) return 0;
  if (fm)
    ctr_fwd_kernel<true><<<(B + 3) / 4, 256, 0, st>>>(ids, dense, deep, wide, X, wide_sum, ssum, fm, B, S, D, n_dense,
                                                        ldx, rows);
  else
    ctr_fwd_kernel<false><<<(B + 3) / 4, 256, 0, st>>>(ids, dense, deep, wide, X, wide_sum, ssum, fm, B, S, D,
                                                         n_dense, ldx, rows);
  return 0;
}

long long ctr_part_floats(long long N, int D) { return ((N + CTR_SEG - 1) / CTR_SEG) * 2 * (2LL * D + 4); }

template <int G, bool FM, int MODE>
static void ctr_bwd_launch(const CtrBwdArgs& A, hipStream_t st) {
  const int per = 256 / G, grid = (A.N + per - 1) / per;
  ctr_bwd_rows_kernel<G, FM, MODE><<<grid, 256, 0, st>>>(A);
  ctr_bwd_fold_kernel<G, FM, MODE><<<grid, 256, 0, st>>>(A);
}

template <int G>
static void ctr_bwd_pick(const CtrBwdArgs& A, bool fm, int mode, hipStream_t st) {
  if (mode == CTR_GRAD) {
    if (fm) ctr_bwd_launch<G, true, CTR_GRAD>(A, st);
    else ctr_bwd_launch<G, false, CTR_GRAD>(A, st);
  } else {
    if (fm) ctr_bwd_launch<G, true, CTR_ADAGRAD>(A, st);
    else ctr_bwd_launch<G, false, CTR_ADAGRAD>(A, st);
  }
}

int ctr_bwd_rows(const int64_t* keys, const int64_t* perm, const float* dX, const float* dlogit, const float* ssum,
                 float* part, float* deep, float* wide, float* out_deep, float* out_wide, const float* lr, int B,
                 int S, int D, int ldx, long long rows, int mode, hipStream_t st) {
  if (!ctr_dim_ok(D)) return -2;
  if (B < 0 || S < 1 || rows < 0 || (long long)S * D > ldx || (long long)B * S > 0x7fffffffLL) return -2;
  if (mode != CTR_GRAD && mode != CTR_ADAGRAD) return -2;
  if (mode == CTR_ADAGRAD && lr == nullptr) return -2;
  if (B == 0) return 0;
  const CtrBwdArgs A{keys, perm, dX, dlogit, ssum, part, deep, wide, out_deep, out_wide, lr, B * S, S, D, ldx, rows};
  const int L = D / 4;
  if (L <= 4) ctr_bwd_pick<4>(A, ssum != nullptr, mode, st);
  else if (L <= 8) ctr_bwd_pick<8>(A, ssum != nullptr, mode, st);
  else ctr_bwd_pick<16>(A, ssum != nullptr, mode, st);
  return 0;
}

}  // namespace pdo
