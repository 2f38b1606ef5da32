// SPDX-License-Identifier: Apache-2.0
// C[M][N] = bf16(Σ_k (A[m][k]·2^(S[m][k/32] − 127))·B[n][k] · db (+ bias[N]) (+ res[M][N])) on gfx950: A as MXFP8
// rows — OCP e4m3 bytes with one E8M0 scale byte per 32 consecutive k, as gemm_nt_f8's fc1 epilogue writes them
// (gemm_nt_f8.hip, MX) — B per-tensor e4m3 bytes with its device float db (quant_f8.hip), fp32 accumulation, one
// rounding at the bf16 store.  This is GPT-2's fc2 on FP8: its input never exists as a whole row in one place, so
// a per-token scale cannot be taken, a per-block one can.
//
// MFMA: v_mfma_scale_f32_16x16x128_f8f6f4, both operands e4m3.  The instruction scales its k order in blocks of
// 32: block b of row r by 2^(byte − 127), the byte taken from the scale register of lane 16b + r and selected by
// op_sel (a compile-time field, the same for all lanes).  Measured with one-hot operands on the MI355X
// (profiles/fp8_mx.md): a lane's byte does NOT go with the 32 values that lane holds.  In the instruction's k
// order lane l's first four registers are k 16(l >> 4) .. + 15 and its last four k 64 + 16(l >> 4) .. + 15, so
// block b is the first halves of lane groups 2b, 2b + 1 (b < 2) or the second halves of groups 2(b − 2),
// 2(b − 2) + 1.  The fragment map follows that: lane l holds row l & 15 and the 16-B chunks (l >> 4) and
// 4 + (l >> 4) of the k-tile (gemm_nt_f8 takes 2(l >> 4) and 2(l >> 4) + 1; unscaled, any map that is the same
// for A and B does), and for fragment i of k-tile kt the lane carries block l >> 4's byte,
// S[m0 + 128·wm + 16i + (l & 15)][4·kt + (l >> 4)].  It is loaded as a byte (global_load_ubyte: the register's
// byte 0, op_sel 0, no shift), 8 loads per lane and k-tile against 64 MFMAs.  B's scale register holds 0x7f (2^0)
// in every lane; db joins in the epilogue's fma.
//
// Everything else is gemm_nt_f8's and is described there: 256 × 256 tile, 4 waves each owning 128 × 128 as 64
// pinned 16×16 accumulators, BK = 128, the [buffer][A|B][256][128 B] LDS image with chunk c of row r at
// c ^ ((r >> 1) & 7) written by LDS-DMA with the swizzle on the source, B's rows permuted so a lane's accumulators
// are 8 consecutive columns, one barrier per k-tile, one flat k-tile stream across a workgroup's output tiles,
// persistent XCD-remapped grid.  The scale bytes do not go through LDS (1 KiB per k-tile): the 8 loads of k-tile
// t + 1 are issued in step t's slots 17 – 24, right behind the 16 DMA pieces, into the register set step t does
// not read (two sets of 8, indexed by the buffer).  They count in vmcnt like the DMA, and the vm_wait<0>() at the
// head of step t + 1 covers both.  The last step of a tile loads the next tile's k-tile 0 scales with its DMA.
//
// Epilogues: EPI_PLAIN, EPI_BIAS as gemm_nt_f8 stores them, and EPI_BIAS_ADD: x = fma(acc, db, bias) + res in
// fp32, rounded once — fc2 joining the residual stream.  The residual rows are 16-B loads straight into registers
// (no LDS staging): a lane's (i, e) row piece is the 8 columns it stores.  Blocks i = 0, 1 are requested before the
// tile's last k-tile and arrive under its MFMAs; block i + 2 is requested when block i is converted, three
// register sets of 4 × 16 B in rotation.
//
// Shape rule: gemm_nt_f8's (M % 256 = 0, N % 256 ∈ {0, 128}, K % 256 = 0, K ≥ 256); S dense with row stride K / 32.
#include <type_traits>
#include <utility>

#include "cdna4.h"
#include "gemm_nt_epi.h"
#include "kernels.h"

namespace pdo {

namespace {

constexpr int BM = 256, BN = 256, BK = 128, NTHR = 256;
constexpr int OPB = 256 * BK;  // bytes of one operand tile [256][128] fp8 = 32 KiB

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// pinned-accumulator scaled MFMA under cdna4.h's rules (mfma16_acc); sa / sb: the lanes' E8M0 bytes in byte 0.
// The scale registers come from loads (sa) or are written once at kernel entry (sb): no VALU write in front.
__device__ __forceinline__ void mfma_mx8_acc(f32x4& c, const i32x8& a, const i32x8& b, unsigned sa, unsigned sb) {
  asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel:[0,0,0] op_sel_hi:[0,0,0]"
               : "+a"(c)
               : "v"(a), "v"(b), "v"(sa), "v"(sb));
}
__device__ __forceinline__ void mfma_mx8_acc0(f32x4& c, const i32x8& a, const i32x8& b, unsigned sa, unsigned sb) {
  asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, 0, %3, %4 op_sel:[0,0,0] op_sel_hi:[0,0,0]"
               : "=a"(c)
               : "v"(a), "v"(b), "v"(sa), "v"(sb));
}

// one scale byte, zero-extended; the pointer is global memory (said so: behind srcs()'s asm hipcc would load flat)
__device__ __forceinline__ unsigned ld_u8(const unsigned char* p) {
  return *(const __attribute__((address_space(1))) unsigned char*)p;
}

constexpr bool epi_mx8(int e) { return epi_plain_store(e) || e == EPI_BIAS_ADD; }

template <int EPI>
__global__ __launch_bounds__(NTHR, 1) void gemm_nt_mx8_kernel(const unsigned char* __restrict__ A,
                                                              const unsigned char* __restrict__ S,
                                                              const unsigned char* __restrict__ B, int lda, int ldb,
                                                              int lds, int M, int N, int nk, bf16* __restrict__ C,
                                                              int ldc, const bf16* __restrict__ bias,
                                                              const bf16* __restrict__ res, int ldr,
                                                              const float* __restrict__ db, int group_m) {
  static_assert(epi_mx8(EPI), "no such epilogue");
  constexpr bool ADD = EPI == EPI_BIAS_ADD;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * OPB];  // [buf][A|B][256][128]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int tiles_n = (N + BN - 1) / BN;  // N % 256 = 128 allowed (half-width last tile column)
  const int nwg = (M / BM) * tiles_n;
  const float scale = db[0];
  auto coords = [&](int v, int& tm_, int& tn_) {  // gemm_nt4's tile order
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
  bool halfn = n0 + BN > N;  // only N − n0 = 128 columns exist: the wn = 1 waves load no residual and store nothing

  // ---- LDS-DMA sources and pieces: gemm_nt_f8's
  const int rb = lane >> 3;
  const int csrc = (lane & 7) ^ (4 * (w & 1) + (lane >> 4));
  const unsigned voffA = (unsigned)(rb * lda + csrc * 16);
  const unsigned voffB = (unsigned)(8 * rb * ldb + csrc * 16);
  const unsigned stepA = (unsigned)(32 * lda), stepB = (unsigned)(2 * ldb);
  const unsigned lds0 = lds_addr(smem) + (unsigned)(w * 1024);
  struct Src {
    const unsigned char* a;
    const unsigned char* b;
    const unsigned char* s;  // the k-tile's scale bytes of the tile's first row
    unsigned hi;             // B row step of the pieces' upper half (0 on a half-width tile)
  };
  auto srcs = [&](int m0_, int n0_, int kt) {
    Src r{A + ((size_t)m0_ + 8 * w) * lda + (size_t)kt * BK,
          B + ((size_t)n0_ + 64 * (w & 1) + (w >> 1)) * ldb + (size_t)kt * BK, S + (size_t)m0_ * lds + 4 * kt,
          n0_ + BN > N ? 0u : 64u};
    asm volatile("" : "+s"(r.a), "+s"(r.b), "+s"(r.s), "+s"(r.hi));  // bases formed beside each use, not kept live
    return r;
  };
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

  // ---- fragment reads: rows (l & 15) of block i / j, k chunks (l >> 4) and 4 + (l >> 4): the halves of MX blocks
  // (l >> 4) >> 1 and 2 + ((l >> 4) >> 1) the instruction expects in this lane (head)
  const int sw = (lane >> 1) & 7, g4 = lane >> 4;
  const int cA = (g4 ^ sw) << 4, cB = ((4 + g4) ^ sw) << 4;
  const int ra = (wm * 128 + (lane & 15)) * BK, rbb = OPB + (wn * 128 + (lane & 15)) * BK;
  auto rd = [&](auto buf_tag, int row_off) -> i32x8 {
    constexpr int BUF = decltype(buf_tag)::value;
    const unsigned char* p = smem + BUF * 2 * OPB + row_off;
    const i32x4 lo = *reinterpret_cast<const i32x4*>(p + cA);
    const i32x4 hi = *reinterpret_cast<const i32x4*>(p + cB);
    return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  // ---- scale bytes: fragment i's is at soff + 16·i·lds past Src::s (row 128·wm + 16i + (l & 15), block l >> 4:
  // this lane supplies the block's byte, other lanes hold the block's values)
  const unsigned soff = (unsigned)((wm * 128 + (lane & 15)) * lds + g4);
  const unsigned sstep = (unsigned)(16 * lds);
  unsigned sa[2][8];  // [buffer of the k-tile][i]
  unsigned sb = 0x7fu;
  asm volatile("" : "+v"(sb));  // one register for all 64 MFMAs, not an inline constant per use

  f32x4 acc[8][8];  // first written by mfma_mx8_acc0 in each tile's k-tile 0
  i32x8 fa[8], fb[8];
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;

  // slot s = MFMA (i, j) = (s >> 3, s & 7) of one k-tile in buffer BUF:
  //   before 0   vmcnt(0), barrier; reads A 0, B 0-2
  //   s 0-4      read B s + 3            s 1-16   DMA piece s − 1 of `next` (when load)
  //   s 8i + 2   read A i + 1 (i < 7)    s 17-24  scale byte s − 17 of `next` (when load)
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
      if constexpr (FIRST) mfma_mx8_acc0(acc[i][j], fa[i], fb[j], sa[BUF][i], sb);
      else mfma_mx8_acc(acc[i][j], fa[i], fb[j], sa[BUF][i], sb);
      if constexpr (s < 5) fb[s + 3] = rd(SB{}, rbb + (s + 3) * 2048);
      if constexpr (j == 2 && i < 7) fa[i + 1] = rd(SB{}, ra + (i + 1) * 2048);
      if constexpr (s >= 1 && s <= 16) {
        if (load) dma(next, NB{}, s - 1);
      }
      if constexpr (s >= 17 && s <= 24) {
        if (load) sa[BUF ^ 1][s - 17] = ld_u8(next.s + (soff + (unsigned)(s - 17) * sstep));
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
  // acc[i][j][e] = product[m][n], m = wm·128 + 16i + 4(l >> 4) + e, n = wn·128 + 8(l & 15) + j: per (i, e) a lane
  // stores 8 consecutive columns, non-temporal, and (EPI_BIAS_ADD) reads the same 8 of res
  bf16x8 rv[ADD ? 3 : 1][4];
  auto load_res = [&](int i, int set) {
    if constexpr (ADD) {
      if (halfn && wn == 1) return;
      const bf16* p = res + (size_t)(m0 + wm * 128 + 4 * g4 + 16 * i) * ldr + (n0 + wn * 128 + 8 * (lane & 15));
#pragma unroll
      for (int e = 0; e < 4; ++e) rv[set][e] = *reinterpret_cast<const bf16x8*>(p + (size_t)e * ldr);
    }
  };
  auto epilogue = [&]() {
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");  // XDL D → v_accvgpr_read (hipcc does not pad the asm)
    if (halfn && wn == 1) return;
    const int nb = n0 + wn * 128 + 8 * (lane & 15);
    const size_t mr = (size_t)(m0 + wm * 128 + 4 * g4);
    f32x8 bv8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (epi_needs_bias(EPI)) bv8 = to_f32(*reinterpret_cast<const bf16x8*>(bias + nb));
    const f32x8 sc8 = {scale, scale, scale, scale, scale, scale, scale, scale};
    static_for<8>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      if constexpr (i + 2 < 8) load_res(i + 2, (i + 2) % 3);
      f32x4 a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = rd_acc(acc[i][j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x8 v = {a[0][e], a[1][e], a[2][e], a[3][e], a[4][e], a[5][e], a[6][e], a[7][e]};
        f32x8 x = __builtin_elementwise_fma(v, sc8, bv8);  // the scaled product joins the bias unrounded
        if constexpr (ADD) x += to_f32(rv[i % 3][e]);
        __builtin_nontemporal_store(to_bf16(x), reinterpret_cast<bf16x8*>(C + (mr + 16 * i + e) * ldc + nb));
      }
    });
  };

  using T_ = std::true_type;
  using F_ = std::false_type;
  {
    const Src s0 = srcs(m0, n0, 0);
#pragma unroll
    for (int p = 0; p < 16; ++p) dma(s0, B0{}, p);
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[0][i] = ld_u8(s0.s + (soff + (unsigned)i * sstep));
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
    load_res(0, 0);
    load_res(1, 1);
    step(B1{}, F_{}, srcs(ntm * BM, ntn * BN, 0), has_next);  // the next tile's k-tile 0 under this one's last
    epilogue();
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

int gemm_nt_mx8(const unsigned char* A, const unsigned char* S, const unsigned char* B, const float* db, int M, int N,
                int K, int lda, int ldb, bf16* C, int ldc, int epi, const bf16* bias, const bf16* res, int ldr,
                hipStream_t st) {
  if (!gemm_nt_f8_ok(M, N, K, lda, ldb, ldc)) return -2;
  if (!S || !db) return -3;
  if (epi_mx8(epi))
    if (const int rc = gemm_nt_args_rc(epi, bias != nullptr, res != nullptr, ldr, N, false, false)) return rc;
  const long long tiles = (long long)(M / BM) * ((N + BN - 1) / BN);
  if (tiles > 0x7fffffffLL) return -2;
  constexpr int group_m = 4;  // gemm_nt4's
  return nt_epi_dispatch(std::integer_sequence<int, EPI_PLAIN, EPI_BIAS, EPI_BIAS_ADD>{}, epi, [&](auto e) {
    gemm_nt_mx8_kernel<decltype(e)::value><<<persistent_grid(tiles), NTHR, 0, st>>>(
        A, S, B, lda, ldb, K / 32, M, N, K / BK, C, ldc, bias, res, ldr, db, group_m);
    return 0;
  });
}

}  // namespace pdo
