// SPDX-License-Identifier: Apache-2.0
// C[M][N] = bf16((A[M][K] · B[N][K]ᵀ) · da · db (+ bias[N])) on gfx950, A and B
// OCP e4m3 bytes (quant_f8.hip), da / db device floats (powers of two), fp32
// accumulation, one rounding at the bf16 store.  EPI_PLAIN and EPI_BIAS.
//
// Row form (gemm_nt_f8_kernel<EPI, true>): da holds M floats, one per row of A — the
// per-token scales of the e4m3 rows a LayerNorm wrote (layernorm.hip, Q8); db
// stays one float.  The store is still one fma, C = bf16(fma(acc, da[m]·db,
// bias)); da[m]·db is an exact power of two while it stays normal (both are
// 2^−e with |e| ≤ 126, so the product can leave the normal range only when
// both operands are extreme — then it rounds like any fp32 product).  A lane's
// rows are mr + 16i + e: per i the four da[mr + 16i .. + 3] are one 16-B load,
// requested before the tile's last k-tile.  On this form the kernel also has
// fc1's epilogue EPI_GELU_SAVE_GRAD, as gemm_nt4 stores it: x = fma(acc, da[m]·db,
// bias), C = bf16(gelu'(x)), Y = bf16(gelu(x)) (common.h, gelu_and_grad2).
//
// MX (gemm_nt_f8_kernel<EPI_GELU_SAVE_GRAD, true, true>): that epilogue also writes the bf16-rounded Y as MXFP8
// rows for gemm_nt_mx8 (fc2): Q[M][N] e4m3 bytes and S[M][N / 32] E8M0 bytes 127 − e, both dense row-major, e by
// quant_f8.hip's rule over each block of 32 consecutive columns (f8_quant.h).  Per (i, e) a lane holds 8
// consecutive columns of one row, so a block is a quad of lanes: amax on the |bits| of the bf16 values with two
// DPP quad_perm steps, one multiply and f8_cvt8, an 8-B non-temporal store per lane and row.  A wave's 128
// columns are four blocks: their bytes are gathered into one dword by two DPP row rotations and stored by one
// lane per row (N % 128 = 0: 4-B aligned).  The other instantiations' code does not change.
//
// Work split: gemm_nt4's — 256 × 256 output tile, 4 waves, one per SIMD, each
// owning a 128 × 128 block as 64 16×16 accumulators pinned to the accumulator
// file; persistent one-workgroup-per-CU grid with the XCD remap and the grouped
// tile order.  BK = 128 fp8, so an operand tile is the 32 KiB of gemm_nt4's 64
// bf16 and the LDS image carries over in byte terms: [buffer][A|B][256 rows]
// [128 B], 16-B chunk c of row r at chunk c ^ ((r >> 1) & 7), written linearly
// by the LDS-DMA with the swizzle on the source address, B's rows permuted
// (physical row 128h + q holds row 128h + 8(q & 15) + (q >> 4)) so that a lane's
// accumulators are 8 consecutive output columns and the epilogue stores 16 B
// per lane straight from registers.
//
// MFMA: v_mfma_f32_16x16x128_f8f6f4 (cbsz = blgp = 0: both operands e4m3), one
// per (i, j) block and k-tile, 16 passes each: 64 MFMAs per k-tile do the work
// of gemm_nt4's 128.  A lane holds 32 k bytes of its row: row l & 15, the 16-B
// chunks 2(l >> 4) and 2(l >> 4) + 1, two ds_read_b128 per fragment.  A and B
// fragments take the same chunks, and a dot product does not depend on the
// order of k, so only the row ↔ lane map matters; it is that of the bf16
// 16×16×32 form (SrcA rows → 4 consecutive accumulator rows per lane, SrcB rows
// → lane & 15).  The unscaled form is used: no E8M0 operand to carry.
//
// Schedule: one barrier per k-tile and one flat stream of k-tiles across the
// output tiles of a workgroup.  Step t waits for its own DMA pieces, passes the
// barrier (which also says every wave has read k-tile t − 1, whose fragment
// reads its MFMAs have consumed), then issues the 16 pieces of the next k-tile
// into the other buffer — the next OUTPUT tile's first k-tile when t is the
// last of this one, so that load flies under the last 64 MFMAs and the
// epilogue.  Runs of 8 MFMAs share the A fragment; the fragments are read in
// consumption order a few slots ahead (B 3 slots, A 6), so per k-tile only the
// first reads' latency and the barrier are exposed (≈ 5 % of its 4096 MFMA
// cycles).  This is simpler than gemm_nt4's three-barrier operand-split refill
// on purpose: with MFMAs twice as long, a whole k-tile of lead covers the DMA
// with two buffers.  Measured (profiles/fp8_qkv.md, [65536, C] → 3C): 1.85 /
// 2.16 / 2.26 PF at C = 768 / 1024 / 1280 against gemm_nt4's 1.13 / 1.26 / 1.32.
// Accumulation: on quantised Gaussian data the result stays inside ½ bf16 ulp +
// K·2⁻²⁴·Σ|a·b| of the float64 product (worst ratio 0.91), i.e. the f8f6f4 MFMA
// behaves as fp32 sums; on integer operands it is exact.
//
// K rule: K % 256 = 0, K ≥ 256 (k-tiles run in pairs, which keeps the buffer
// index static; one pair is enough for this schedule, so the 256-wide smoke
// model runs the kernel too).
#include <type_traits>
#include <utility>

#include "cdna4.h"
#include "f8_quant.h"
#include "gemm_nt_epi.h"
#include "kernels.h"

namespace pdo {

namespace {

constexpr int BM = 256, BN = 256, BK = 128, NTHR = 256;
constexpr int OPB = 256 * BK;  // bytes of one operand tile [256][128] fp8 = 32 KiB

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// pinned-accumulator MFMA under cdna4.h's rules (mfma16_acc): operands from
// ds_read, first write with C = 0, rewritten 64 MFMAs later, epilogue pads
__device__ __forceinline__ void mfma_f8_acc(f32x4& c, const i32x8& a, const i32x8& b) {
  asm volatile("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_f8_acc0(f32x4& c, const i32x8& a, const i32x8& b) {
  asm volatile("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, 0" : "=a"(c) : "v"(a), "v"(b));
}

// the epilogues this kernel has: the plain stores on either scale form, fc1's on the row form
constexpr bool epi_f8(int e, bool rows) { return epi_plain_store(e) || (rows && e == EPI_GELU_SAVE_GRAD); }
static_assert(epi_f8(EPI_PLAIN, false) && epi_f8(EPI_BIAS, false) && !epi_f8(EPI_GELU_SAVE_GRAD, false) &&
              epi_f8(EPI_PLAIN, true) && epi_f8(EPI_BIAS, true) && epi_f8(EPI_GELU_SAVE_GRAD, true) &&
              !epi_f8(EPI_GELU, true) && !epi_f8(EPI_BIAS_ADD, true) && !epi_f8(EPI_STATS, true),
              "gemm_nt_f8's epilogue list");

struct NoOut {};  // the trailing kernel argument of the scalar form
struct RowsOut {  // of the row form: EPI_GELU_SAVE_GRAD's second output
  bf16* Y;
  int ldy;
};
struct MxOut : RowsOut {  // MX: Y's rows once more as MXFP8, dense: Q[M][N] e4m3 bytes, S[M][N / 32] E8M0 bytes
  unsigned char* Q;
  unsigned char* S;
};

// ROWS = false: da is one float; true: M floats, one per row of A (per token)
// MX (fc1's epilogue on the row form only): also write bf16(Y) as MXFP8 rows for gemm_nt_mx8
template <int EPI, bool ROWS = false, bool MX = false>
__global__ __launch_bounds__(NTHR, 1) void gemm_nt_f8_kernel(const unsigned char* __restrict__ A,
                                                             const unsigned char* __restrict__ B, int lda, int ldb,
                                                             int M, int N, int nk, bf16* __restrict__ C, int ldc,
                                                             const bf16* __restrict__ bias,
                                                             const float* __restrict__ da,
                                                             const float* __restrict__ db, int group_m,
                                                             std::conditional_t<MX, MxOut, std::conditional_t<ROWS, RowsOut, NoOut>> yo) {
  static_assert(epi_f8(EPI, ROWS), "no such epilogue");
  static_assert(!MX || (ROWS && EPI == EPI_GELU_SAVE_GRAD), "MXFP8 rows come from fc1's epilogue");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * OPB];  // [buf][A|B][256][128]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int tiles_n = (N + BN - 1) / BN;  // N % 256 = 128 allowed (half-width last tile column)
  const int nwg = (M / BM) * tiles_n;
  const float scale = ROWS ? db[0] : da[0] * db[0];  // exact: powers of two (ROWS: da[m] joins in the epilogue)
  // gemm_nt4's tile order: XCD-contiguous ids, group_m tile rows per column step
  auto coords = [&](int v, int& tm_, int& tn_) {
    const int id = xcd_remap(v, nwg);
    const int tiles_m = M / BM, per_group = group_m * tiles_n;
    const int g = id / per_group, first_m = g * group_m;
    const int gsz = min(tiles_m - first_m, group_m), r = id - g * per_group;
    tm_ = first_m + r % gsz;
    tn_ = r / gsz;
  };
  int vcur = blockIdx.x, tm, tn;
  coords(vcur, tm, tn);
  int m0 = tm * BM, n0 = tn * BN;
  bool halfn = n0 + BN > N;  // only N − n0 = 128 columns exist: the wn = 1 waves store nothing

  // ---- LDS-DMA sources (gemm_nt4's, in bytes).  Wave w fills the 8-row blocks
  // w + 4p (p = 0..7) of both operands; lane l → physical row 8(w + 4p) + (l >> 3),
  // LDS chunk l & 7, global chunk (l & 7) ^ swz(row), swz = 4(w & 1) + (l >> 4).
  // B: that physical row holds row 128(p >> 2) + 64(w & 1) + (w >> 1) + 2(p & 3)
  // + 8(l >> 3); a half-width tile's upper half re-reads the lower half (in bounds).
  const int rb = lane >> 3;
  const int csrc = (lane & 7) ^ (4 * (w & 1) + (lane >> 4));
  const unsigned voffA = (unsigned)(rb * lda + csrc * 16);
  const unsigned voffB = (unsigned)(8 * rb * ldb + csrc * 16);
  const unsigned stepA = (unsigned)(32 * lda), stepB = (unsigned)(2 * ldb);
  const unsigned lds0 = lds_addr(smem) + (unsigned)(w * 1024);
  struct Src {
    const unsigned char* a;
    const unsigned char* b;
    unsigned hi;  // B row step of the pieces' upper half (0 on a half-width tile)
  };
  auto srcs = [&](int m0_, int n0_, int kt) {
    Src r{A + ((size_t)m0_ + 8 * w) * lda + (size_t)kt * BK,
          B + ((size_t)n0_ + 64 * (w & 1) + (w >> 1)) * ldb + (size_t)kt * BK, n0_ + BN > N ? 0u : 64u};
    asm volatile("" : "+s"(r.a), "+s"(r.b), "+s"(r.hi));  // bases formed beside each DMA, not kept live
    return r;
  };
  // piece p of a k-tile into buffer BUF: p < 8 → A block w + 4p, else B block w + 4(p − 8)
  auto dma = [&](const Src& sr, auto buf_tag, int p) {
    constexpr int BUF = decltype(buf_tag)::value;
    const unsigned base = lds0 + (unsigned)(BUF * 2 * OPB);
    if (p < 8) {
      glds16(voffA, sr.a + p * stepA, base + (unsigned)(4096 * p));
    } else {
      const int pp = p - 8;
      glds16(voffB, sr.b + ((unsigned)(pp & 3) + sr.hi * (unsigned)(pp >> 2)) * stepB, base + OPB + (unsigned)(4096 * pp));
    }
  };

  // ---- fragment reads: rows (l & 15) of block i / j, k chunks 2(l >> 4), 2(l >> 4) + 1
  const int sw = (lane >> 1) & 7, g4 = lane >> 4;
  const int cA = ((2 * g4) ^ sw) << 4, cB = ((2 * g4 + 1) ^ sw) << 4;
  const int ra = (wm * 128 + (lane & 15)) * BK, rbb = OPB + (wn * 128 + (lane & 15)) * BK;
  auto rd = [&](auto buf_tag, int row_off) -> i32x8 {
    constexpr int BUF = decltype(buf_tag)::value;
    const unsigned char* p = smem + BUF * 2 * OPB + row_off;
    const i32x4 lo = *reinterpret_cast<const i32x4*>(p + cA);
    const i32x4 hi = *reinterpret_cast<const i32x4*>(p + cB);
    return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };

  f32x4 acc[8][8];  // first written by mfma_f8_acc0 in each tile's k-tile 0
  i32x8 fa[8], fb[8];
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;

  // slot s = MFMA (i, j) = (s >> 3, s & 7) of one k-tile in buffer BUF:
  //   before 0   vmcnt(0), barrier; reads A 0, B 0-2
  //   s 0-4      read B s + 3            s 1-16  DMA piece s − 1 of `next` (when load)
  //   s 8i + 2   read A i + 1 (i < 7)
  auto step = [&](auto buf_tag, auto first_tag, const Src& next, bool load) {
    constexpr int BUF = decltype(buf_tag)::value;
    constexpr bool FIRST = decltype(first_tag)::value;
    using SB = std::integral_constant<int, BUF>;
    using NB = std::integral_constant<int, BUF ^ 1>;
    vm_wait<0>();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    fa[0] = rd(SB{}, ra);
    fb[0] = rd(SB{}, rbb);
    fb[1] = rd(SB{}, rbb + 2048);
    fb[2] = rd(SB{}, rbb + 2 * 2048);
    __builtin_amdgcn_sched_barrier(0);
    static_for<64>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      constexpr int i = s >> 3, j = s & 7;
      if constexpr (FIRST) mfma_f8_acc0(acc[i][j], fa[i], fb[j]);
      else mfma_f8_acc(acc[i][j], fa[i], fb[j]);
      if constexpr (s < 5) fb[s + 3] = rd(SB{}, rbb + (s + 3) * 2048);
      if constexpr (j == 2 && i < 7) fa[i + 1] = rd(SB{}, ra + (i + 1) * 2048);
      if constexpr (s >= 1 && s <= 16) {
        if (load) dma(next, NB{}, s - 1);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  auto rd_acc = [](const f32x4& a) {
    f32x4 v;
    asm volatile("v_accvgpr_read_b32 %0, %4\n\tv_accvgpr_read_b32 %1, %5\n\tv_accvgpr_read_b32 %2, %6\n\tv_accvgpr_read_b32 %3, %7"
                 : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3])
                 : "a"(a[0]), "a"(a[1]), "a"(a[2]), "a"(a[3]));
    return v;
  };
  // acc[i][j][e] = product[m][n], m = wm·128 + 16i + 4(l >> 4) + e, n = wn·128 +
  // 8(l & 15) + j: per (i, e) a lane stores 8 consecutive columns, non-temporal
  // ROWS: the tile's row scales, one 16-B load per i (rows mr + 16i .. + 3 of this lane), requested before the
  // tile's last k-tile so that they arrive under its 64 MFMAs (M % 256 = 0: every row exists)
  f32x4 dav[ROWS ? 8 : 1];
  auto load_row_scales = [&]() {
    if constexpr (ROWS) {
      const float* p = da + (m0 + wm * 128 + 4 * g4);
#pragma unroll
      for (int i = 0; i < 8; ++i) dav[i] = *reinterpret_cast<const f32x4*>(p + 16 * i);
    }
  };
  auto row_epilogue = [&]() {
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");  // XDL D → v_accvgpr_read (hipcc does not pad the asm)
    if (halfn && wn == 1) return;
    const int nb = n0 + wn * 128 + 8 * (lane & 15);
    const size_t mr = (size_t)(m0 + wm * 128 + 4 * g4);
    f32x8 bv8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (epi_needs_bias(EPI)) bv8 = to_f32(*reinterpret_cast<const bf16x8*>(bias + nb));
    const f32x8 sc8 = {scale, scale, scale, scale, scale, scale, scale, scale};
    f32x2 m1 = {-1.f, -1.f};
    if constexpr (EPI == EPI_GELU_SAVE_GRAD) asm volatile("" : "+v"(m1));  // common.h, gelu_sig_grad2
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      f32x4 a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = rd_acc(acc[i][j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x8 v = {a[0][e], a[1][e], a[2][e], a[3][e], a[4][e], a[5][e], a[6][e], a[7][e]};
        if constexpr (!ROWS) {
          // one fma: the scaled product joins the bias unrounded
          const bf16x8 o = to_bf16(__builtin_elementwise_fma(v, sc8, bv8));
          __builtin_nontemporal_store(o, reinterpret_cast<bf16x8*>(C + (mr + 16 * i + e) * ldc + nb));
          continue;
        }
        const float s = dav[ROWS ? i : 0][e] * scale;  // da[m]·db
        const f32x8 x = __builtin_elementwise_fma(v, f32x8{s, s, s, s, s, s, s, s}, bv8);
        bf16* crow = C + (mr + 16 * i + e) * ldc + nb;
        if constexpr (EPI == EPI_GELU_SAVE_GRAD) {
          // fc1 as gemm_nt4 stores it: C = gelu'(x), Y = gelu(x), x the fp32 pre-activation
          f32x8 y, g;
#pragma unroll
          for (int q = 0; q < 8; q += 2) {
            f32x2 yy, gg;
            gelu_and_grad2(f32x2{x[q], x[q + 1]}, m1, yy, gg);
            y[q] = yy[0];
            y[q + 1] = yy[1];
            g[q] = gg[0];
            g[q + 1] = gg[1];
          }
          __builtin_nontemporal_store(to_bf16(g), reinterpret_cast<bf16x8*>(crow));
          const bf16x8 yb = to_bf16(y);
          __builtin_nontemporal_store(yb, reinterpret_cast<bf16x8*>(yo.Y + (mr + 16 * i + e) * yo.ldy + nb));
          if constexpr (MX) {
            // the 32-column block of this row is the quad of lanes around this one: amax on the |bits| of the
            // bf16-rounded values (an integer max orders them as floats), two quad_perm steps
            const u16x8 ub = __builtin_bit_cast(u16x8, yb) & (unsigned short)0x7fff;
            int am = max(max(max((int)ub[0], (int)ub[1]), max((int)ub[2], (int)ub[3])),
                         max(max((int)ub[4], (int)ub[5]), max((int)ub[6], (int)ub[7])));
            am = max(am, __builtin_amdgcn_mov_dpp(am, 0xb1, 0xf, 0xf, false));  // quad_perm:[1,0,3,2]
            am = max(am, __builtin_amdgcn_mov_dpp(am, 0x4e, 0xf, 0xf, false));  // quad_perm:[2,3,0,1]
            const int ex = f8_scale_exp((unsigned)am << 16);
            const float sx = f8_pow2(ex);
            const size_t row = mr + 16 * i + e;
            const i32x2 qv = f8_cvt8(to_f32(yb) * f32x8{sx, sx, sx, sx, sx, sx, sx, sx});
            __builtin_nontemporal_store(qv, reinterpret_cast<i32x2*>(yo.Q + row * (size_t)N + nb));
            // the wave's four scale bytes of this row (127 − e, block b in byte b) gathered by two rotations of the
            // 16-lane row — an OR over lanes l, l ± 4, l ± 8, l ± 12 whichever way it turns — and stored as one dword
            int sw4 = (127 - ex) << (8 * ((lane >> 2) & 3));
            sw4 |= __builtin_amdgcn_mov_dpp(sw4, 0x124, 0xf, 0xf, false);  // row_ror:4
            sw4 |= __builtin_amdgcn_mov_dpp(sw4, 0x128, 0xf, 0xf, false);  // row_ror:8
            if ((lane & 15) == 0) *reinterpret_cast<int*>(yo.S + row * (size_t)(N >> 5) + ((n0 + wn * 128) >> 5)) = sw4;
          }
        } else {
          __builtin_nontemporal_store(to_bf16(x), reinterpret_cast<bf16x8*>(crow));
        }
      }
    }
  };

  using T_ = std::true_type;
  using F_ = std::false_type;
  {
    const Src s0 = srcs(m0, n0, 0);
#pragma unroll
    for (int p = 0; p < 16; ++p) dma(s0, B0{}, p);
  }
  for (;;) {
    // nk is even and ≥ 2 (host contract): pairs keep the buffer index static
    step(B0{}, T_{}, srcs(m0, n0, 1), true);
    for (int t = 1; t < nk - 1; t += 2) {
      step(B1{}, F_{}, srcs(m0, n0, t + 1), true);
      step(B0{}, F_{}, srcs(m0, n0, t + 2), true);
    }
    const int vnext = vcur + (int)gridDim.x;
    const bool has_next = vnext < nwg;
    int ntm = tm, ntn = tn;
    if (has_next) coords(vnext, ntm, ntn);
    load_row_scales();
    step(B1{}, F_{}, srcs(ntm * BM, ntn * BN, 0), has_next);  // the next tile's k-tile 0 under this one's last
    row_epilogue();
    if (!has_next) break;
    vcur = vnext;
    tm = ntm;
    tn = ntn;
    m0 = tm * BM;
    n0 = tn * BN;
    halfn = n0 + BN > N;
  }
}

// one workgroup per CU (a multiple of 8: the XCD mapping)
int persistent_grid(long long tiles) {
  static const int ncu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    return n >= 8 ? n / 8 * 8 : 8;
  }();
  return (int)(tiles < ncu ? tiles : ncu);
}

}  // namespace

int gemm_nt_f8_ok(int M, int N, int K, int lda, int ldb, int ldc) {
  return M > 0 && N > 0 && M % BM == 0 && (N % BN == 0 || N % BN == BN / 2) && K >= 2 * BK && K % (2 * BK) == 0 &&
         lda % 16 == 0 && ldb % 16 == 0 && lda >= K && ldb >= K && ldc % 4 == 0 && ldc >= N;
}

int gemm_nt_f8(const unsigned char* A, const float* da, const unsigned char* B, const float* db, int M, int N, int K,
               int lda, int ldb, bf16* C, int ldc, int epi, const bf16* bias, hipStream_t st, bool da_rows, bf16* Y,
               int ldy, unsigned char* Q, unsigned char* S) {
  if (!gemm_nt_f8_ok(M, N, K, lda, ldb, ldc)) return -2;
  if (!da || !db || (da_rows && reinterpret_cast<uintptr_t>(da) % 16)) return -3;
  // gemm_nt()'s verdict on the epilogue's own arguments (bias, Y, ldy); the 4-wave-only fc1 epilogue exists here
  // on the row form alone
  if (epi_f8(epi, true))
    if (const int rc = gemm_nt_args_rc(epi, bias != nullptr, Y != nullptr, ldy, N, false, da_rows)) return rc;
  const long long tiles = (long long)(M / BM) * ((N + BN - 1) / BN);
  if (tiles > 0x7fffffffLL) return -2;
  constexpr int group_m = 4;  // gemm_nt4's
  const int g = persistent_grid(tiles);
  if (Q || S) {  // fc1's epilogue with the MXFP8 copy of Y
    if (!da_rows || epi != EPI_GELU_SAVE_GRAD) return -4;
    if (!Q || !S || reinterpret_cast<uintptr_t>(Q) % 8 || reinterpret_cast<uintptr_t>(S) % 4) return -3;
    gemm_nt_f8_kernel<EPI_GELU_SAVE_GRAD, true, true><<<g, NTHR, 0, st>>>(A, B, lda, ldb, M, N, K / BK, C, ldc, bias, da,
                                                                          db, group_m, MxOut{{Y, ldy}, Q, S});
    return 0;
  }
  if (da_rows)
    return nt_epi_dispatch(std::integer_sequence<int, EPI_PLAIN, EPI_BIAS, EPI_GELU_SAVE_GRAD>{}, epi, [&](auto e) {
      gemm_nt_f8_kernel<decltype(e)::value, true><<<g, NTHR, 0, st>>>(A, B, lda, ldb, M, N, K / BK, C, ldc, bias, da, db,
                                                                      group_m, RowsOut{Y, ldy});
      return 0;
    });
  return nt_epi_dispatch(std::integer_sequence<int, EPI_PLAIN, EPI_BIAS>{}, epi, [&](auto e) {
    gemm_nt_f8_kernel<decltype(e)::value><<<g, NTHR, 0, st>>>(A, B, lda, ldb, M, N, K / BK, C, ldc, bias, da, db, group_m,
                                                              NoOut{});
    return 0;
  });
}

}  // namespace pdo
