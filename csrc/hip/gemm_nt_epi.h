// SPDX-License-Identifier: Apache-2.0
// The forward GEMM's fused epilogues (gemm_nt.hip, gemm_nt4.hip): their names, what each needs and writes, the
// argument check and the runtime → template dispatch.  constexpr host / device code only; the two static_assert
// tables at the end are the contract, checked at every build.  What each epilogue computes: gemm_nt.hip's head.
#pragma once
#include <utility>

namespace pdo {

// the values are the kernels' `int EPI` template arguments (an enum-typed parameter would rename every kernel)
enum NtEpi : int {
  EPI_PLAIN, EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_ADD, EPI_BIAS_ADD, EPI_ADD_MASKED, EPI_GELU_SAVE_GRAD, EPI_DGELU_SAVED,
  EPI_STATS, EPI_COUNT
};

constexpr bool epi_known(int e) { return e >= 0 && e < EPI_COUNT; }
constexpr bool epi_bias_into_c(int e) { return e == EPI_BIAS || e == EPI_BIAS_ADD; }  // bias joins the stored product
constexpr bool epi_bias_into_activation(int e) { return e == EPI_GELU || e == EPI_DGELU || e == EPI_GELU_SAVE_GRAD; }
// the `bias` argument is read (EPI_ADD_MASKED: as the addend's keep-mask bytes, 8 columns each)
constexpr bool epi_needs_bias(int e) { return epi_bias_into_c(e) || epi_bias_into_activation(e) || e == EPI_ADD_MASKED; }
constexpr bool epi_reads_y(int e) { return e == EPI_DGELU || (e >= EPI_ADD && e <= EPI_ADD_MASKED) || e == EPI_DGELU_SAVED; }
constexpr bool epi_writes_y(int e) { return e == EPI_GELU || e == EPI_GELU_SAVE_GRAD; }
constexpr bool epi_col_partials(int e) { return e == EPI_DGELU || e == EPI_DGELU_SAVED; }  // fp32 bias-gradient rows
constexpr bool epi_stats(int e) { return e == EPI_STATS; }                                  // BatchNorm partial rows
constexpr bool epi_nt4_only(int e) { return e == EPI_GELU_SAVE_GRAD || e == EPI_DGELU_SAVED; }
constexpr bool epi_plain_store(int e) { return e == EPI_PLAIN || e == EPI_BIAS; }  // C = bf16(product (+ bias)), no more

// gemm_nt()'s verdict on an epilogue's arguments: 0, -3 (a needed argument is missing or misaligned) or -4 (no
// such epilogue on this mainloop; nt4 = the 4-wave one runs this K).  A value past the list is asked for Y before
// it is refused, as the range check this replaces did.
constexpr int gemm_nt_args_rc(int epi, bool have_bias, bool have_y, int ldy, int N, bool have_part, bool nt4) {
  if (epi_needs_bias(epi) && !have_bias) return -3;
  if (epi == EPI_ADD_MASKED && ldy % 8) return -3;  // rows of whole mask bytes
  if ((epi_reads_y(epi) || epi_writes_y(epi) || epi >= EPI_COUNT) && (!have_y || ldy % 4 || ldy < N)) return -3;
  if ((epi_col_partials(epi) || epi_stats(epi)) && !have_part) return -3;
  if (epi_nt4_only(epi) && !nt4) return -4;
  return epi_known(epi) ? 0 : -4;
}

// fn(std::integral_constant<int, E>{}) for the E of the list that equals epi; -4 when none does.  (A recursion, not a
// fold: hipcc emits the kernels a fold instantiates in reverse order, and the assembly is compared as text.)
template <class F>
int nt_epi_dispatch(std::integer_sequence<int>, int, F&&) { return -4; }
template <int E, int... Es, class F>
int nt_epi_dispatch(std::integer_sequence<int, E, Es...>, int epi, F&& fn) {
  return epi == E ? fn(std::integral_constant<int, E>{}) : nt_epi_dispatch(std::integer_sequence<int, Es...>{}, epi, fn);
}

constexpr bool epi_row(int e, int value, bool bias, bool to_c, bool to_act, bool rd_y, bool wr_y, bool colp, bool stats,
                       bool nt4, bool plain) {
  return e == value && epi_needs_bias(e) == bias && epi_bias_into_c(e) == to_c && epi_bias_into_activation(e) == to_act &&
         epi_reads_y(e) == rd_y && epi_writes_y(e) == wr_y && epi_col_partials(e) == colp && epi_stats(e) == stats &&
         epi_nt4_only(e) == nt4 && epi_plain_store(e) == plain;
}
// gemm_nt_args_rc at N = 256: 0 with all it may need (bias, Y with ldy = N, partial rows, the 4-wave mainloop), and
// the code with one of them taken away or another ldy (0: the epilogue does not need it)
constexpr bool epi_args_row(int e, int no_bias, int no_y, int ldy_m4, int ldy_p2, int ldy_p4, int no_part, int no_nt4) {
  return gemm_nt_args_rc(e, 1, 1, 256, 256, 1, 1) == 0 && gemm_nt_args_rc(e, 0, 1, 256, 256, 1, 1) == no_bias &&
         gemm_nt_args_rc(e, 1, 0, 256, 256, 1, 1) == no_y && gemm_nt_args_rc(e, 1, 1, 252, 256, 1, 1) == ldy_m4 &&
         gemm_nt_args_rc(e, 1, 1, 258, 256, 1, 1) == ldy_p2 && gemm_nt_args_rc(e, 1, 1, 260, 256, 1, 1) == ldy_p4 &&
         gemm_nt_args_rc(e, 1, 1, 256, 256, 0, 1) == no_part && gemm_nt_args_rc(e, 1, 1, 256, 256, 1, 0) == no_nt4;
}
// clang-format off
//                                               needs  bias  bias   reads  writes  column    stats  4-wave  plain
//                                        value  bias   → C   → act  Y      Y       partials         only    store
static_assert(epi_row(EPI_PLAIN,          0,     0,     0,    0,     0,     0,      0,        0,     0,      1));
static_assert(epi_row(EPI_BIAS,           1,     1,     1,    0,     0,     0,      0,        0,     0,      1));
static_assert(epi_row(EPI_GELU,           2,     1,     0,    1,     0,     1,      0,        0,     0,      0));
static_assert(epi_row(EPI_DGELU,          3,     1,     0,    1,     1,     0,      1,        0,     0,      0));
static_assert(epi_row(EPI_ADD,            4,     0,     0,    0,     1,     0,      0,        0,     0,      0));
static_assert(epi_row(EPI_BIAS_ADD,       5,     1,     1,    0,     1,     0,      0,        0,     0,      0));
static_assert(epi_row(EPI_ADD_MASKED,     6,     1,     0,    0,     1,     0,      0,        0,     0,      0));
static_assert(epi_row(EPI_GELU_SAVE_GRAD, 7,     1,     0,    1,     0,     1,      0,        0,     1,      0));
static_assert(epi_row(EPI_DGELU_SAVED,    8,     0,     0,    0,     1,     0,      1,        0,     1,      0));
static_assert(epi_row(EPI_STATS,          9,     0,     0,    0,     0,     0,      0,        1,     0,      0));
//                                             no     no   ldy    ldy    ldy    no        off the
//                                             bias   Y    N - 4  N + 2  N + 4  partials  4-wave mainloop
static_assert(epi_args_row(EPI_PLAIN,           0,    0,    0,     0,     0,     0,        0));
static_assert(epi_args_row(EPI_BIAS,           -3,    0,    0,     0,     0,     0,        0));
static_assert(epi_args_row(EPI_GELU,           -3,   -3,   -3,    -3,     0,     0,        0));
static_assert(epi_args_row(EPI_DGELU,          -3,   -3,   -3,    -3,     0,    -3,        0));
static_assert(epi_args_row(EPI_ADD,             0,   -3,   -3,    -3,     0,     0,        0));
static_assert(epi_args_row(EPI_BIAS_ADD,       -3,   -3,   -3,    -3,     0,     0,        0));
static_assert(epi_args_row(EPI_ADD_MASKED,     -3,   -3,   -3,    -3,    -3,     0,        0));
static_assert(epi_args_row(EPI_GELU_SAVE_GRAD, -3,   -3,   -3,    -3,     0,     0,       -4));
static_assert(epi_args_row(EPI_DGELU_SAVED,     0,   -3,   -3,    -3,     0,    -3,       -4));
static_assert(epi_args_row(EPI_STATS,           0,    0,    0,     0,     0,    -3,        0));
// clang-format on
static_assert(gemm_nt_args_rc(EPI_DGELU_SAVED, 1, 1, 256, 256, 0, 0) == -3, "-3 comes before -4");
static_assert(gemm_nt_args_rc(-1, 1, 1, 256, 256, 1, 1) == -4 && gemm_nt_args_rc(EPI_COUNT, 1, 1, 256, 256, 1, 1) == -4 &&
              gemm_nt_args_rc(EPI_COUNT, 1, 0, 256, 256, 1, 1) == -3, "values outside the list");

}  // namespace pdo
