// SPDX-License-Identifier: Apache-2.0
// Weight-gradient GEMM C[M][N] (+)= Σ_t A[t][M] · B[t][N] on gfx950 — the
// 4-wave, one-wave-per-SIMD mainloop (same contract as gemm_dw.hip, selected
// by gemm_dw_set_impl).  The operand handling is gemm_dw's: token-major tiles
// staged into LDS as they lie in memory (LDS-DMA, swizzle on the source
// address) and every fragment read with ds_read_b64_tr_b16; the schedule is
// gemm_nt4's (profiles/r2_gemm_nt4.md): each wave owns 128 × 128 outputs = 256
// accumulator registers, pinned to the accumulator file, and one instruction
// stream per wave interleaves MFMAs, transposed reads and DMA.
//
// The schedule (dw4_tile, written once for both MFMA shapes): tile t (64 tokens,
// LDS buffer t & 1) is two 32-token blocks of 16 MFMA groups, two barriers per
// tile.  Each 32-token half of a buffer is refilled with tile t+2 as soon as every
// wave has read it — the first half during block 0 of tile t (after barrier B0:
// F0(t) reads done), the second during block 1 (after B1: F1(t) reads done).  Tile
// t+1's data therefore has ≈ 1.5 tiles of lead (issued during tile t-1, first read
// after B1 of tile t) instead of ≈ 0.5, at the price of two barriers per tile
// (hipBLASLt's gfx950 loop does the same with three).
//
// RAW / WAR: a buffer half is refilled only after the barrier that follows
// every wave's last read of it; a tile is read only after every wave retired
// its own DMA of it and passed a barrier.  (Round 4 housekeeping: the
// one-barrier schedules of round 2 measured slower and were removed,
// profiles/r2_gemm_nt4.md.)
//
// The two kernels run it on the two MFMA shapes; they differ in the LDS swizzle
// (dw_tile.h), the fragment addressing (rd), the accumulators a group touches (mma)
// and the epilogue:
//   gemm_dw4_kernel     v_mfma_f32_32x32x16_bf16, 4 × 4 accumulators of 32 × 32, a
//                       block is two k-steps of 4 A + 4 B fragments (A/B alternative);
//   gemm_dw4m16_kernel  v_mfma_f32_16x16x32_bf16, 8 × 8 accumulators of 16 × 16, a
//                       block is ONE k-step of 8 A + 8 B fragments (the default; also
//                       the convolution weight gradient and the grouped launch).
// Their set-up and prologue stay written out per kernel: moved into a shared
// forced-inline body, hipcc compiles every kernel differently
// (profiles/r14_dw4_one_mainloop.md).
#include <type_traits>

#include "dw_tile.h"
#include "kernels.h"

namespace pdo {

namespace {

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int LROW = 256;             // LDS row (elements) of a [BK][256] tile
constexpr int TILE = BK * LROW;       // elements per operand tile
constexpr int OPB = TILE * 2;         // bytes per operand tile (32 KiB)
constexpr int NTHR = 256;
using Tile = DwTile<LROW>;            // the 32x32x16 variant's swizzle and fragments (dw_tile.h)

// One tile of the schedule: tile t lies in LDS buffer BUF, f0 holds its block 0
// (tokens 0-31).  Block 0's 16 MFMA groups run while block 1 is read into f1 and, with
// EOUT, the first half of tile t+2 is DMAed over block 0's rows; block 1's groups run
// while (MORE) tile t+1's block 0 is read into f0 and the second half follows.
// mma(first_tag, f, g): the shape's MFMAs of group g on fragments f; FIRST: the
// accumulators' first write.  Pieces: first half = A 0-3, B 8-11; second = A 4-7, B 12-15.
template <int BUF, bool MORE, bool FIRST, bool EOUT, class Srcs, class Dma, class Rd, class Mma>
__device__ __forceinline__ void dw4_tile(int t, Srcs& srcs, Dma& dma, Rd& rd, Mma& mma, bf16x8 (&f0)[16],
                                         bf16x8 (&f1)[16]) {
  using NB = std::integral_constant<int, BUF ^ 1>;
  using SB = std::integral_constant<int, BUF>;
  decltype(srcs(0)) sn2{};
  if constexpr (EOUT) sn2 = srcs(t + 2);
  // B0: every wave's F0(t) reads (buffer BUF, tokens 0-31) are done
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    mma(std::bool_constant<FIRST>{}, f0, g);
    f1[g] = rd(SB{}, 1, g);
    if constexpr (EOUT) {
      if (g & 1) dma(sn2, SB{}, (g >> 1) < 4 ? (g >> 1) : (g >> 1) + 4);  // first-half pieces
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // B1: every wave's F1(t) reads are done (tokens 32-63 of BUF free) and tile t+1
  // has landed (only tile t+2's first-half pieces may still fly)
  if constexpr (MORE || EOUT) {
    if constexpr (EOUT)
      asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    mma(std::false_type{}, f1, g);
    if constexpr (MORE) f0[g] = rd(NB{}, 0, g);
    if constexpr (EOUT) {
      if (g & 1) dma(sn2, SB{}, (g >> 1) < 4 ? (g >> 1) + 4 : (g >> 1) + 8);  // second-half pieces
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Workgroup → output tile (tm, tn) and split of a split-K launch, and the split's
// k-tiles [k0, k0 + nk).  M % 256 == 128: a half-height last row of tiles.  k-tiles
// are dealt to the splits in pairs (the mainloop runs tiles in pairs): the first
// P % splits slices take one pair more.
__device__ __forceinline__ void dw4_slice(int M, int N, int splits, int ksteps_total, int& tm, int& tn, int& split,
                                          int& k0, int& nk) {
  const int tiles_n = N / BN, tiles_m = (M + BM - 1) / BM;
  const int nwg = tiles_m * tiles_n * splits;
  const int id = xcd_remap((int)blockIdx.x, nwg);
  tn = id % tiles_n;
  tm = (id / tiles_n) % tiles_m;
  split = id / (tiles_n * tiles_m);
  const int pq = (ksteps_total >> 1) / splits, pr = (ksteps_total >> 1) % splits;
  k0 = 2 * (split * pq + min(split, pr));
  nk = 2 * (pq + (split < pr ? 1 : 0));
}

__global__ __launch_bounds__(NTHR, 1) void gemm_dw4_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B,
                                                           int lda, int ldb, int M, int N, int ksteps_total,
                                                           int splits, bf16* __restrict__ C, int ldc,
                                                           long long split_stride, int accumulate) {
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * 2 * TILE];  // [buf][A|B][BK][256]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  int tm, tn, split, k0, nk;
  dw4_slice(M, N, splits, ksteps_total, tm, tn, split, k0, nk);
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- LDS-DMA: a wave-instruction fills 1 KiB = 2 token rows of 512 B.  Wave
  // w's piece i (0..7) of an operand covers rows 2(4i + w) + (l >> 5), LDS chunk
  // l & 31 holding global chunk (l & 31) ^ 4·(row & 3); row & 3 = (2w + (l >> 5))
  // & 3 is fixed per lane.  Per-lane byte offset in a VGPR, wave-uniform base
  // (k-tile, piece) in SGPRs.
  const int rl = lane >> 5;
  const int cs = (lane & 31) ^ (((2 * w + rl) & 3) << 2);
  // half-height edge tile (columns m0 + 128 .. m0 + 255 of A do not exist): those
  // lanes re-fetch columns m0 .. m0 + 127 — in bounds, and the rows they feed are
  // never stored
  const int csa = (m0 + BM > M && cs >= 16) ? cs - 16 : cs;
  const unsigned voffA = (unsigned)((rl * lda + csa * 8) * 2), voffB = (unsigned)((rl * ldb + cs * 8) * 2);
  const bf16* baseA = A + ((size_t)k0 * BK + 2 * w) * lda + m0;
  const bf16* baseB = B + ((size_t)k0 * BK + 2 * w) * ldb + n0;
  const unsigned stepAb = (unsigned)(16 * lda), stepBb = (unsigned)(16 * ldb);  // 8 rows, bytes
  const unsigned lds0 = lds_addr(smem) + (unsigned)(w * 1024);
  // glds16 (M0 not saved around the DMA): nothing else in this kernel uses M0
  struct Src {
    const char* a;
    const char* b;
    unsigned sa, sb;
  };
  auto srcs = [&](int kt) {  // laundered per tile: pieces form their bases with scalar adds
    Src r{reinterpret_cast<const char*>(baseA + (size_t)kt * BK * lda),
          reinterpret_cast<const char*>(baseB + (size_t)kt * BK * ldb), stepAb, stepBb};
    asm volatile("" : "+s"(r.a), "+s"(r.b), "+s"(r.sa), "+s"(r.sb));
    return r;
  };
  auto dma = [&](const Src& sr, auto buf_tag, int p) {  // p < 8: A piece p, else B piece p - 8
    constexpr int BUF = decltype(buf_tag)::value;
    const unsigned base = lds0 + (unsigned)(BUF * 2 * OPB);
    if (p < 8) glds16(voffA, sr.a + p * sr.sa, base + (unsigned)(4096 * p));
    else glds16(voffB, sr.b + (p - 8) * sr.sb, base + OPB + (unsigned)(4096 * (p - 8)));
  };

  // ---- fragments: block half h (0: tokens 0-31, 1: 32-63) holds k-steps 2h, 2h+1;
  // slot q (0..15) = k-step q >> 3, operand (q & 7) < 4 ? A mb : B nb
  const bf16* smA[2] = {smem, smem + 2 * TILE};
  int fa[4], fb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    fa[i] = Tile::frag_base(wm * 128 + 32 * i, lane);
    fb[i] = TILE + Tile::frag_base(wn * 128 + 32 * i, lane);
  }
  auto rd = [&](auto buf_tag, int h, int q) -> bf16x8 {
    constexpr int BUF = decltype(buf_tag)::value;
    const bf16* T = smA[BUF] + ((q & 7) < 4 ? fa[q & 3] : fb[q & 3]);
    const int ks = 2 * h + (q >> 3);
    switch (ks) {
      case 0: return Tile::frag<0>(T);
      case 1: return Tile::frag<16>(T);
      case 2: return Tile::frag<32>(T);
      default: return Tile::frag<48>(T);
    }
  };
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;

  f32x16 acc[4][4];  // first written with FIRST in tile 0's block 0
  bf16x8 f0[16], f1[16];

  {
    {
      const Src s0 = srcs(0), s1 = srcs(1);
#pragma unroll
      for (int p = 0; p < 16; ++p) dma(s0, B0{}, p);
#pragma unroll
      for (int p = 0; p < 16; ++p) dma(s1, B1{}, p);
    }
    vm_wait<16>();  // tile 0 landed (tile 1 may fly)
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 16; ++q) f0[q] = rd(B0{}, 0, q);
    auto mma = [&](auto first_tag, const bf16x8* f, int g) {
      // group g: k-step g >> 3, A fragment (g >> 1) & 3 against B fragments 2(g & 1), +1
      constexpr bool FIRST = decltype(first_tag)::value;
      const int ks = g >> 3, mb = (g >> 1) & 3, nb0 = 2 * (g & 1);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (FIRST && ks == 0) mfma32_acc0(acc[mb][nb0 + u], f[8 * ks + mb], f[8 * ks + 4 + nb0 + u]);
        else mfma32_acc(acc[mb][nb0 + u], f[8 * ks + mb], f[8 * ks + 4 + nb0 + u]);
      }
    };
    auto tileH = [&](int t, auto buf_tag, auto more_tag, auto first_tag, auto eout_tag) {
      dw4_tile<decltype(buf_tag)::value, decltype(more_tag)::value, decltype(first_tag)::value,
               decltype(eout_tag)::value>(t, srcs, dma, rd, mma, f0, f1);
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    tileH(0, B0{}, T_{}, T_{}, T_{});
    tileH(1, B1{}, T_{}, F_{}, T_{});
    for (int t = 2; t < nk - 2; t += 2) {
      tileH(t, B0{}, T_{}, F_{}, T_{});
      tileH(t + 1, B1{}, T_{}, F_{}, T_{});
    }
    tileH(nk - 2, B0{}, T_{}, F_{}, F_{});
    tileH(nk - 1, B1{}, F_{}, F_{}, F_{});
  }

  // ---- epilogue: acc[mb][nb][r] = C[m0 + wm·128 + 32mb + (r&3) + 8(r>>2) + 4hh][n0 + wn·128 + 32nb + (l&31)]
  // the accumulators leave through explicit v_accvgpr_read, padded against the
  // last MFMAs (hipcc does not see into the asm): 16 wait states
  asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
  bf16* Cb = C + (size_t)split * split_stride;
  const int hh = lane >> 5, li = lane & 31;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v[r]) : "a"(acc[mb][nb][r]));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 128 + 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (m >= M) continue;  // edge tile: wave-uniform (wm = 1 holds rows m0 + 128 ..)
        const int n = n0 + wn * 128 + 32 * nb + li;
        bf16* p = Cb + (size_t)m * ldc + n;
        float x = v[r];
        if (accumulate) x += (float)*p;
        *p = (bf16)x;
      }
    }
}

// ============================================================================
// The half-buffer-refill schedule on v_mfma_f32_16x16x32_bf16 (variant 0, the default).
// Same tile (256 × 256 per workgroup, 128 × 128 per wave), same DMA and
// barriers; each wave's outputs are 8 × 8 accumulators of 16 × 16 (still 256
// AGPRs), a 32-token block is ONE k-step (8 A + 8 B fragments, 64 MFMAs of
// half the 32x32x16 cycles).  Why: on random bf16 data the chip holds a higher
// clock on the 16x16x32 shape — MI355X_MICROARCH.md 'DVFS give-back' item 7
// (1.12-1.15x FLOP/s at equal cycles per FLOP in LDS-fed loops).
//
// The tile swizzle and fragment layout of this shape: dw_tile.h (DwTile16); the DMA's
// source-side swizzle depends on the piece's parity (row bit 3): two per-lane offsets
// per operand.
using Tile16 = DwTile16<LROW>;  // this shape's swizzle and fragments (dw_tile.h)

// GATHER (the convolution weight gradient, conv.hip's conv_wgrad): B is not a
// token-major matrix but the NHWC activation gathered per tap — column
// tap·C + ci of token t is x[pixel(t, tap)][ci], zero for a padding pixel (a
// buffer_load … lds whose offset is pushed past the buffer) — and the output
// is fp32 partials [split][M][N] (folded by conv_wgrad_reduce in split order).
struct DwGather {
  const bf16* x;
  unsigned xbytes;
  int C, S, IH, IW, TA, TB;  // forward output grid: token t = (n·TA + ho)·TB + wo
  int TC;                    // R·S·C: columns past it (padding to the 256-column tile) read zeros
  float inv_TA, inv_TB;
  int st, pad;
  float* part;
};

// GROUPED: several independent problems in one launch (gemm_dw4_grouped), each
// workgroup one output tile over its problem's whole token axis.  The table is a
// kernel argument; first[i] = tiles of problems 0 .. i-1.
struct DwGroupEntry {
  const bf16* A;
  const bf16* B;
  bf16* C;
  int lda, ldb, ldc, M, N, ksteps, accumulate;
};
struct DwGroupTable {
  int n;
  int first[DW_GROUP_MAX + 1];
  DwGroupEntry p[DW_GROUP_MAX];
};
struct DwNoGroup {};

// Grouped workgroup id → tile of the concatenated problems.  The hardware deals
// workgroup b to XCD b & 7, and an XCD's 32 CUs hold its slots 32r .. 32r + 31
// together: those 32 get consecutive tiles (the last, partial round of 256 is dealt
// as xcd_remap deals a whole grid).
__device__ __forceinline__ int dw_group_tile(int b, int total) {
  const int full = total & ~255;
  if (b < full) return (b & ~255) + ((b & 7) << 5) + ((b >> 3) & 31);
  return full + xcd_remap(b - full, total - full);
}
// Tile t of a problem → (tm, tn): strips of 4 tile columns, row-major inside a
// strip, so 32 consecutive tiles are an 8 × 4 block where the shape has one (two
// 4 × 4 blocks side by side for a 4-row problem); the last strip may be narrower.
__device__ __forceinline__ void dw_group_mn(int t, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int fulls = tiles_n >> 2, per = 4 * tiles_m;
  if (t < fulls * per) {
    const int s = t / per, r = t - s * per;
    tm = r >> 2;
    tn = 4 * s + (r & 3);
  } else {
    const int r = t - fulls * per, wd = tiles_n & 3;
    tm = r / wd;
    tn = 4 * fulls + r - tm * wd;
  }
}

// SWAP (the grouped launch): the MFMA takes the x fragment as its row operand, so a
// lane's 4 accumulator registers are 4 adjacent columns of one output row (one 8-B
// store) instead of 4 rows of one column; the products and their order are the same.
// The split-K instantiation keeps its layout: with short slices the wide stores
// measured no faster there (16 single GEMMs: 5105 vs 5064 us, profiles/r13_grouped_dw.md).
template <bool GATHER, bool GROUPED>
__global__ __launch_bounds__(NTHR, 1) void gemm_dw4m16_kernel(
    const bf16* __restrict__ A_, const bf16* __restrict__ B_, int lda_, int ldb_, int M_, int N_, int ksteps_total,
    int splits, bf16* __restrict__ C_, int ldc_, long long split_stride, int accumulate_, const DwGather gx,
    const std::conditional_t<GROUPED, DwGroupTable, DwNoGroup> tb) {
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * 2 * TILE];  // [buf][A|B][BK][256]
  constexpr bool SWAP = GROUPED;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const bf16* A = A_;
  const bf16* B = B_;
  bf16* C = C_;
  int lda = lda_, ldb = ldb_, ldc = ldc_, M = M_, N = N_, accumulate = accumulate_;
  int tm, tn, split, k0, nk;
  if constexpr (GROUPED) {
    const int g = dw_group_tile((int)blockIdx.x, tb.first[tb.n]);
    int pi = 0;
    while (g >= tb.first[pi + 1]) ++pi;  // ≤ DW_GROUP_MAX scalar steps
    const DwGroupEntry& e = tb.p[pi];
    A = e.A, B = e.B, C = e.C;
    lda = e.lda, ldb = e.ldb, ldc = e.ldc, M = e.M, N = e.N, accumulate = e.accumulate;
    dw_group_mn(g - tb.first[pi], (M + BM - 1) / BM, N / BN, tm, tn);
    split = 0, k0 = 0, nk = e.ksteps;
  } else {
    dw4_slice(M, N, splits, ksteps_total, tm, tn, split, k0, nk);
  }
  const int m0 = tm * BM, n0 = tn * BN;

  // LDS-DMA: piece i of an operand = rows 8i + 2w + rl (rl = l >> 5), LDS chunk
  // l & 31 ← global chunk (l & 31) ^ Tile16::swz(row); the swizzle of that row is fixed per
  // lane up to the piece parity (row bit 3 = i & 1)
  const int rl = lane >> 5, rw = 2 * w + rl;
  unsigned voffA[2], voffB[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int cs = (lane & 31) ^ Tile16::swz(8 * par + rw);
    const int csa = (m0 + BM > M && cs >= 16) ? cs - 16 : cs;  // half-height edge tile (see gemm_dw4_kernel)
    voffA[par] = (unsigned)((rl * lda + csa * 8) * 2);
    voffB[par] = (unsigned)((rl * ldb + cs * 8) * 2);
  }
  const bf16* baseA = A + ((size_t)k0 * BK + 2 * w) * lda + m0;
  const bf16* baseB = GATHER ? A : B + ((size_t)k0 * BK + 2 * w) * ldb + n0;
  const unsigned stepAb = (unsigned)(16 * lda), stepBb = (unsigned)(16 * ldb);
  const unsigned lds0 = lds_addr(smem) + (unsigned)(w * 1024);  // glds16 / bufld16_lds: no other M0 use here either
  // GATHER: per parity, the lane's column chunk → (tap row / column offset, channel)
  int gdh[2] = {0, 0}, gdw[2] = {0, 0}, gci[2] = {0, 0};
  const __amdgpu_buffer_rsrc_t rsX = buf_rsrc(GATHER ? gx.x : A, GATHER ? (int)gx.xbytes : 0);
  if constexpr (GATHER) {
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      const int col = n0 + (((lane & 31) ^ Tile16::swz(8 * par + rw)) << 3);
      const int tap = col / gx.C, r = tap / gx.S;
      gci[par] = col - tap * gx.C;
      gdh[par] = col < gx.TC ? r - gx.pad : -(1 << 20);  // a padding column fails every bounds check
      gdw[par] = tap - r * gx.S - gx.pad;
    }
  }
  struct Src {
    const char* a;
    const char* b;
    unsigned sa, sb;
    int kt;
  };
  auto srcs = [&](int kt) {
    Src r{reinterpret_cast<const char*>(baseA + (size_t)kt * BK * lda),
          reinterpret_cast<const char*>(baseB + (GATHER ? 0 : (size_t)kt * BK * ldb)), stepAb, stepBb, kt};
    asm volatile("" : "+s"(r.a), "+s"(r.b), "+s"(r.sa), "+s"(r.sb));
    return r;
  };
  auto dma = [&](const Src& sr, auto buf_tag, int p) {  // p < 8: A piece p, else B piece p - 8
    constexpr int BUF = decltype(buf_tag)::value;
    const unsigned base = lds0 + (unsigned)(BUF * 2 * OPB);
    if (p < 8) {
      glds16(voffA[p & 1], sr.a + p * sr.sa, base + (unsigned)(4096 * p));
    } else if constexpr (GATHER) {
      // B piece p - 8: token rows 8(p - 8) + 2w + rl of k-tile k0 + kt
      const int t = (k0 + sr.kt) * BK + 8 * (p - 8) + rw;
      int q, wo, n, ho;
      divmod(t, gx.TB, gx.inv_TB, q, wo);
      divmod(q, gx.TA, gx.inv_TA, n, ho);
      const int hi = ho * gx.st + gdh[p & 1], wi = wo * gx.st + gdw[p & 1];
      const unsigned off = ((unsigned)hi < (unsigned)gx.IH && (unsigned)wi < (unsigned)gx.IW)
                               ? (unsigned)((((n * gx.IH + hi) * gx.IW + wi) * gx.C + gci[p & 1]) * 2)
                               : 0x80000000u;
      bufld16_lds(off, rsX, base + OPB + (unsigned)(4096 * (p - 8)));
    } else {
      glds16(voffB[p & 1], sr.b + (p - 8) * sr.sb, base + OPB + (unsigned)(4096 * (p - 8)));
    }
  };

  // fragment slot q (0..15) of block h (tokens 32h .. 32h+31): q < 8 → A rows
  // wm·128 + 16q, else B columns wn·128 + 16(q - 8)
  const bf16* smA[2] = {smem, smem + 2 * TILE};
  int fo[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    fo[i] = Tile16::frag_base(wm * 128 + 16 * i, lane);
    fo[8 + i] = TILE + Tile16::frag_base(wn * 128 + 16 * i, lane);
  }
  auto rd = [&](auto buf_tag, int h, int q) -> bf16x8 {
    constexpr int BUF = decltype(buf_tag)::value;
    const bf16* T = smA[BUF] + fo[q];
    return h ? Tile16::frag<32>(T) : Tile16::frag<0>(T);
  };
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;

  f32x4 acc[8][8];  // first written with FIRST in tile 0's block 0
  bf16x8 f0[16], f1[16];

  {
    const Src s0 = srcs(0), s1 = srcs(1);
#pragma unroll
    for (int p = 0; p < 16; ++p) dma(s0, B0{}, p);
#pragma unroll
    for (int p = 0; p < 16; ++p) dma(s1, B1{}, p);
  }
  vm_wait<16>();  // tile 0 landed (tile 1 may fly)
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 16; ++q) f0[q] = rd(B0{}, 0, q);
  auto mma = [&](auto first_tag, const bf16x8* f, int g) {
    // group g: A fragment g >> 1 against B fragments 4(g & 1) .. +3
    constexpr bool FIRST = decltype(first_tag)::value;
    const int mb = g >> 1, nb0 = 4 * (g & 1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bf16x8& fr = f[SWAP ? 8 + nb0 + u : mb];
      const bf16x8& fc = f[SWAP ? mb : 8 + nb0 + u];
      if (FIRST) mfma16_acc0(acc[mb][nb0 + u], fr, fc);
      else mfma16_acc(acc[mb][nb0 + u], fr, fc);
    }
  };
  auto tileH = [&](int t, auto buf_tag, auto more_tag, auto first_tag, auto eout_tag) {
    dw4_tile<decltype(buf_tag)::value, decltype(more_tag)::value, decltype(first_tag)::value,
             decltype(eout_tag)::value>(t, srcs, dma, rd, mma, f0, f1);
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  tileH(0, B0{}, T_{}, T_{}, T_{});
  tileH(1, B1{}, T_{}, F_{}, T_{});
  for (int t = 2; t < nk - 2; t += 2) {
    tileH(t, B0{}, T_{}, F_{}, T_{});
    tileH(t + 1, B1{}, T_{}, F_{}, T_{});
  }
  tileH(nk - 2, B0{}, T_{}, F_{}, F_{});
  tileH(nk - 1, B1{}, F_{}, F_{}, F_{});

  // ---- epilogue: acc[mb][nb][r] = C[m0 + wm·128 + 16mb + 4(l >> 4) + r][n0 + wn·128 + 16nb + (l & 15)]
  // (with SWAP the lane's row and column roles are exchanged, see the last block)
  asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
  bf16* Cb = C + (size_t)split * split_stride;
  const int g4 = lane >> 4, li = lane & 15;
  if (m0 + wm * 128 >= M) return;  // edge tile: wm = 1 holds rows m0 + 128 .. (wave-uniform)
  if constexpr (GATHER) {
    // fp32 partials of this split (ldc = N)
    float* P = gx.part + (size_t)split * split_stride;
#pragma unroll
    for (int mb = 0; mb < 8; ++mb)
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v[r]) : "a"(acc[mb][nb][r]));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * 128 + 16 * mb + 4 * g4 + r;
          P[(size_t)m * ldc + n0 + wn * 128 + 16 * nb + li] = v[r];
        }
      }
    return;
  }
  if constexpr (!SWAP) {
#pragma unroll
    for (int mb = 0; mb < 8; ++mb)
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v[r]) : "a"(acc[mb][nb][r]));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * 128 + 16 * mb + 4 * g4 + r;
          bf16* p = Cb + (size_t)m * ldc + n0 + wn * 128 + 16 * nb + li;
          float x = v[r];
          if (accumulate) x += (float)*p;
          *p = (bf16)x;
        }
      }
    return;
  }
  // SWAP: acc[mb][nb][r] = C[m0 + wm·128 + 16mb + (l & 15)][n0 + wn·128 + 16nb + 4(l >> 4) + r] —
  // 4 adjacent columns: one 8-B load (accumulate) and one 8-B store per lane, 64 of
  // them where the layout above takes 256 2-B stores (four layers grouped, isolated:
  // 4834 vs 4947 us, profiles/r13_grouped_dw.md)
  const bool al8 = ((reinterpret_cast<size_t>(Cb) | ((size_t)ldc * 2)) & 7) == 0;  // workgroup-uniform
#pragma unroll
  for (int mb = 0; mb < 8; ++mb)
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v[r]) : "a"(acc[mb][nb][r]));
      const int m = m0 + wm * 128 + 16 * mb + li;
      bf16* q = Cb + (size_t)m * ldc + n0 + wn * 128 + 16 * nb + 4 * g4;
      if (al8) {
        bf16x4* p = reinterpret_cast<bf16x4*>(q);
        if (accumulate) {
          const bf16x4 o = *p;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)o[r];
        }
        bf16x4 y;
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = (bf16)v[r];
        *p = y;
      } else {  // a destination or row stride that is not 8-B aligned: element stores
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = v[r];
          if (accumulate) x += (float)q[r];
          q[r] = (bf16)x;
        }
      }
    }
}

}  // namespace

// The slice contract of the mainloop, stated once: k-tiles (64 tokens) run in pairs
// and are dealt to the slices in pairs, the remainder to the first slices, and
// every slice needs ≥ 2 pairs (the prologue fills two tiles, the tail of the loop
// drains two).  Returns the most slices ks k-tiles can be cut into; 0 where not
// even one slice holds (ks odd or < 4).
static long long dw4_max_slices(long long ks) { return ks % 2 ? 0 : ks / 4; }

// Split count of gemm_dw's automatic choice for this mainloop (0: none fits the
// contract): ≤ 256 workgroups (one resident round, one workgroup per CU) unless the
// tiles alone exceed it
int dw4_splits(long long T, int M, int N) {
  const int tiles = ((M + BM - 1) / BM) * (N / BN);
  const long long ks = T / BK;
  if (tiles > 256) {
    // several rounds of one workgroup per CU: the smallest split whose last round
    // is nearly full (LM head, 788 tiles: 1 slice = 3.08 rounds in 4, 4 slices = 12.3 in 13)
    for (int s = 1; s <= 8; ++s) {
      if (s > dw4_max_slices(ks)) continue;
      const long long wg = (long long)tiles * s, rounds = (wg + 255) / 256;
      if (wg * 100 >= rounds * 256 * 94) return s;
    }
  }
  // the most slices that keep one resident round (≤ 256 workgroups): qkv's 48 tiles
  // take 5 uneven slices (240 workgroups) instead of 4 even ones (192)
  for (int s = 16; s >= 1; --s) {
    if ((long long)tiles * s > 256 && s > 1) continue;
    if (s <= dw4_max_slices(ks)) return s;
  }
  return 0;
}

// returns -2 when a slice would break the contract (uneven splits allowed)
int gemm_dw4(const bf16* A, const bf16* B, long long T, int M, int N, int lda, int ldb, bf16* C, int ldc,
             int accumulate, bf16* ws, int splits, hipStream_t st, int variant) {
  if (M % (BM / 2) || N % BN || T % BK || splits < 1 || splits > 16) return -2;
  const long long ks = T / BK;
  if (ks > 0x7fffffffLL || splits > dw4_max_slices(ks)) return -2;
  const int tiles = ((M + BM - 1) / BM) * (N / BN);
  const int grid = tiles * splits;
  bf16* out = C;
  int ldo = ldc;
  long long stride = 0;
  int acc = accumulate;
  if (splits > 1) {
    if (!ws || ldc != N) return -3;
    out = ws;
    ldo = N;
    stride = (long long)M * N;
    acc = 0;
  }
  if (variant == 1)  // the same schedule on 32x32x16 MFMAs (A/B alternative)
    gemm_dw4_kernel<<<grid, NTHR, 0, st>>>(A, B, lda, ldb, M, N, (int)ks, splits, out, ldo, stride, acc);
  else
    gemm_dw4m16_kernel<false, false><<<grid, NTHR, 0, st>>>(A, B, lda, ldb, M, N, (int)ks, splits, out, ldo, stride,
                                                            acc, DwGather{}, DwNoGroup{});
  if (splits > 1) return splitk_add(ws, splits, (long long)M * N, C, accumulate, st);
  return 0;
}

// each problem is one slice
bool gemm_dw4_grouped_ok(long long T, int M, int N) {
  return M > 0 && N > 0 && M % (BM / 2) == 0 && N % BN == 0 && T % BK == 0 && dw4_max_slices(T / BK) >= 1 &&
         T / BK <= 0x7fffffffLL;
}

int gemm_dw4_grouped(const DwProblem* probs, int n, hipStream_t st) {
  if (n < 0) return -2;
  for (int i = 0; i < n; ++i) {
    const DwProblem& q = probs[i];
    if (!gemm_dw4_grouped_ok(q.T, q.M, q.N) || q.lda < q.M || q.ldb < q.N || q.ldc < q.N || !q.A || !q.B || !q.C)
      return -2;
    // per-lane DMA offsets and piece steps are 32-bit byte counts
    if ((long long)q.lda * 16 * 8 >= (1LL << 31) || (long long)q.ldb * 16 * 8 >= (1LL << 31)) return -2;
  }
  for (int i0 = 0; i0 < n;) {
    DwGroupTable tb;
    tb.n = 0;
    tb.first[0] = 0;
    while (i0 < n && tb.n < DW_GROUP_MAX) {
      const DwProblem& q = probs[i0];
      const long long tiles = (long long)((q.M + BM - 1) / BM) * (q.N / BN);
      if (tb.first[tb.n] + tiles > (1 << 24)) {
        if (tb.n == 0) return -2;  // one problem of more than 2^24 tiles
        break;
      }
      tb.p[tb.n] = DwGroupEntry{q.A, q.B, q.C, q.lda, q.ldb, q.ldc, q.M, q.N, (int)(q.T / BK), q.accumulate};
      tb.first[tb.n + 1] = tb.first[tb.n] + (int)tiles;
      ++tb.n;
      ++i0;
    }
    gemm_dw4m16_kernel<false, true><<<tb.first[tb.n], NTHR, 0, st>>>(nullptr, nullptr, 0, 0, 0, 0, 0, 1, nullptr, 0, 0,
                                                                    0, DwGather{}, tb);
  }
  return 0;
}

// Convolution weight gradient on the gathered mainloop: dW [Kout][R·S·C] fp32
// partials per token slice into part ([splits][Kout][TCp], TCp = R·S·C rounded up
// to 256 columns); the caller folds them.  Contract: Kout % 128 = 0, C % 8 = 0,
// tokens % 64 = 0 and the slice contract above.
int conv_wgrad_dw4_splits(int Kout, int TC, long long M) {
  const long long tiles = (long long)((Kout + 255) / 256) * ((TC + 255) / 256);
  static const int ncu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    return n > 0 ? n : 256;
  }();
  // one workgroup per CU (128 KiB of LDS each) and no second round: ⌊CUs / tiles⌋,
  // and no more than the slice contract allows
  const long long ks = M / (2 * BK) * 2;  // whole pairs of k-tiles only
  const long long cap = dw4_max_slices(ks);
  long long sp = ncu / tiles;
  if (sp > cap) sp = cap;
  if (sp > 256) sp = 256;
  return sp < 1 ? 1 : (int)sp;
}

int conv_wgrad_dw4(const bf16* dy, const bf16* x, int N, int H, int W, int C, int Kout, int R, int S, int stride,
                   int pad, float* part, int splits, hipStream_t st) {
  const int Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - S) / stride + 1;
  const long long M = (long long)N * Ho * Wo;
  const int TC = R * S * C, TCp = (TC + BN - 1) / BN * BN;
  if (Kout % (BM / 2) || C % 8 || M % BK || M >= (1LL << 31)) return -2;
  const long long ks = M / BK;
  if (splits < 1 || splits > dw4_max_slices(ks)) return -2;
  if ((long long)N * H * W * C * 2 >= (1LL << 31)) return -2;
  DwGather g{x, (unsigned)((long long)N * H * W * C * 2), C, S, H, W, Ho, Wo, TC, 1.f / (float)Ho, 1.f / (float)Wo,
             stride, pad, part};
  const int grid = ((Kout + BM - 1) / BM) * (TCp / BN) * splits;
  gemm_dw4m16_kernel<true, false><<<grid, NTHR, 0, st>>>(dy, nullptr, Kout, 0, Kout, TCp, (int)ks, splits, nullptr,
                                                         TCp, (long long)Kout * TCp, 0, g, DwNoGroup{});
  return 0;
}

}  // namespace pdo
