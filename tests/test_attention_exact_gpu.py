"""Exact-structure and per-element float64 checks of the plain (no-dropout) flash-attention kernels
of csrc/hip/attention.hip, called straight through the extension (attn_fwd / attn_bwd at thr = 0).
The builders, references and checkers below run on any device; test_attention_exact_cpu.py proves
them on the CPU against an emulation of the arithmetic written down here, and shows that each of a
list of perturbed emulations is rejected.

u = 2^-8 (the bf16 RNE unit roundoff: 8 significant bits, spacing 2^-7 relative, so a rounding moves
a value by up to 2^-8 of itself), U = 2^-24, scale = 1/8, c2 = fp32(log2 e) / 8, HO = 1 + 2^-10 on
every term that is first order in U.  A chain of n products in the matrix unit is charged
2 n U sum|term|: how an MFMA rounds inside has not been measured, the factor 2 is an allowance (at
these shapes the U terms are a few percent of the bf16 terms and decide no check).
  Why not 2^-9, the figure attention.hip's comments give for a bf16 rounding: that is its mean-case
  size, not its bound.  With it the float64 result rounded ONCE misses |got - o| <= Bo + u (|o| +
  Bo) at outputs just above a power of two, and the emulation of the documented arithmetic reaches
  1.2 - 1.6 of the o and dQ bounds in rows of a few keys, where nothing averages.  A counted bound has
  to hold for a faultless kernel, so the roundings are charged at 2^-8.  To give nothing away on top
  of that, a stored bf16 output is not charged a relative u at all: it must lie between
  RNE(v - bound) and RNE(v + bound) (the interval rule of test_ln_gelu_embed_gpu.py), which is exact.

What the kernels compute (read from the code)
    forward   s'_ij = bf16(c2 q_i) . k_j - m, a chain of 64 products onto the accumulator's initial
              -m; m is set by tile 0 and moved only when a 64-key tile exceeds it by more than 8
              (then l and acc are multiplied by alpha = exp2(-d)); P = bf16(exp2(s')), at most 2^8;
              l = fp32 sum of the rounded P; o = RNE(acc rcp(l)); lse = (m + log2 l) ln 2.
    dQ        delta_i = sum_c dO_ic o_ic (fp32 FMAs over the stored bf16 o), lq = fp32(lse log2e);
              P = exp2(fma(q.k, c2, -lq)); dS = bf16(P (dO.v - delta)); dQ = RNE(scale sum_j dS k).
    dK / dV   s' = q_i . bf16(c2 k_j) - lq (the accumulator starts at -lq), dp = dO.v - delta (it
              starts at -delta); P = exp2(s') stays fp32 in the product dS = bf16(P dp) and is
              rounded to bf16 for dV = RNE(sum_i P dO); dK = RNE(scale sum_i dS q).
The three kernels round the score three different ways, so the backward's P does not sum to one;
that is the design.  The backward reference therefore takes the kernel's own forward outputs (R2):
    P_ij = exp(scale q_i.k_j - lse_i),  delta_i = sum_c dO_ic o_ic,  dS = P (dO.v - delta),
    dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO        (float64, lse and o as attn_fwd gave them)
and the forward alone is judged against the true softmax.  Every reference is float64 from the
bf16 inputs as stored (R1); no element of any output is exempt (R3).

Families A1 - A3: every fp32 intermediate is exact (in A3 up to the matrix unit's handling of 2^-46
terms, see there), so the expected bits do not depend on the tile order.  Shapes (B, S, H): (1, 128, 1) the single diagonal block; (2, 256, 3) off-diagonal tiles,
the batch stride and a row stride 3 H 64 that is no power of two; (1, 512, 2) wraps the dK / dV ring
more than once, both parities of the 64-key tile.  Head (b, h) multiplies V or dO by 2^-((b H + h)
mod 4), so exchanged heads show.
  A1  Q = K = 0, V one-hot over the 64-key window at `base`: P = 1, l = q + 1 exactly, and
      o[q, c] = sig RNE(1 / (q + 1)) where base + c <= q, +0 above the diagonal, bit for bit: the
      kernel's fp32 value is (1 / n)(1 + d), |d| <= 3 U (rcp to 1 ulp = 2 U, one multiply), and 1 / n
      lies at least 2^-16.0 (relative) from the nearest bf16 midpoint for every n <= 512 (closest:
      n = 255 and 510; the CPU file asserts it), so "either neighbour" never applies.  lse = ln n
      within 4 U ln n (log2 to 1 ulp = 2 U, the constant ln 2 and the multiply, m = 0).
      Backward from Q = K = V = 0 and dO one-hot over a query window: the dK / dV kernel's
      P~ = exp2(-lq) with lq = fp32(lse log2e) = log2 n (1 + 6 U) is (1 / n)(1 + d), |d| <= (6 ln n +
      2) U <= 2^-18.6, again inside the midpoint distance (asserted per n on the CPU), so
      dV[k, c] = sig RNE(1 / (base + c + 1)) where k <= base + c, else 0; dQ = dK = 0.
  A2  V[k] = a_k e_0 with a fixed random 0 / 1 pattern per head, dO[q] = sig e_0: dP = sig a_k and
      delta_q = sig o[q, 0] are exact (one product each; 1 - o needs 17 bits), so
      dS[q, k] = P~_q sig (a_k - o[q, 0]) with the kernel's own bf16 o.  K one-hot over a key window
      (Q = 0) gives dQ[q, c] = 2^-3 RNE(dS[q, base + c]); Q one-hot over a query window (K = 0) gives
      dK[k, c] = 2^-3 RNE(dS[base + c, k]).  Band rule (check_banded) around the float64
      exp(-lse) sig (a_k - o[q, 0]) with the band (2 |lse| + 3) U |dS|: lq carries 2 U relative (the
      constant log2e and the multiply), that is 2 U |lse| in P; exp2 2 U; the product U.  Entries
      above the diagonal have band 0 and must be 0.  dV[k, 0] = sig RNE(sum_{q >= k} RNE(1 / (q +
      1))) bit for bit (the fp32 sum of those bf16 values is exact: 20 bits), other columns 0.
  A3  Q[q] = 16 e_j(q), K[k] = 16 e_i(k), V = sig x integers in [-8, 8]: a matching pair scores
      16 bf16(16 c2) = 46.25 in log2 units exactly, every other pair 0.  The first matching key
      after tile 0 forces the rescale with alpha = 2^-46.25, then P = 1 on matches and 2^-46.25
      elsewhere, which fp32 absorbs: l = n_match and acc = the integer sum.  Rows without a match
      stay uniform.  o against the float64 softmax under the band rule with the band
      (2 n_i + 3) U (sum_j w_ij |v_jc| + |o_ic|) + 1e-10, n_i = 64 (i / 64 + 1) the products in row i's
      tiles: the P.V chain's allowance, rcp 2 U, the multiply U; the absolute term is the weight of the
      non-matching keys, about 2^-46 x 8 x 512.  The chain term was first left out, on the argument
      that the integer sums are exact and fp32 absorbs the 2^-46 terms.  The matrix unit does not
      absorb them exactly: measured, elements whose matching integers sum to 0 came out at -2^-23 / 3
      (row 28) and -2^-23 (row 37, acc = -2^-21) where exact absorption gives 1e-13 (supposed, not
      measured further: the small products are aligned to the block's largest and cut).  That is the
      internal rounding the allowance is for, so the chain is charged like every other one here; the
      measured loss is 0.2 % of it.
      lse = (46.25 + log2 n_match) ln 2, or ln(q + 1) without a match, within 5 U |lse| (log2 2 U, the
      sum U, the constant and the multiply 2 U): l = n_match exactly (a VALU sum).
      The mix is asserted: at S = 512, 361 rows rescale and 88 rows have no match.
  Band shares.  The share of elements whose band reaches a rounding midpoint is capped at
  A2_CAP = 2 % (expected 2 band / spacing = 2^-11, but dS takes two values per row, so one unlucky row
  is up to 1.5 % of the S = 128 triangle; the CPU emulation has at most 0.39 %) and A3_CAP = 10 % (the
  CPU emulation has 6.6 - 8.0 %: 3 - 4 % are the elements whose integer sum is 0, which the absolute term
  turns into "anything within 1e-10", the rest is the chain allowance); both files assert them.  A1
  has none.
  The 2 GiB slice (S = 128, H = 43691: attn_fwd3_d64<0> and attn_bwd_dq_d64<0>, pointer staging):
  A1 (o, lse, dV) and A2 (dQ) on heads 0, 1, H / 2 and H - 1.

Family B: per element against float64 within counted bounds, on randn, 3 randn (Q, K), the spike of
test_attention_forced_rescale (q = 0.5, one key = 8 mid-sequence off a tile edge), an offset case
(q, k = 2 + 0.1 randn) and the selector inputs; dO is randn.
    A_ij = sum_d |q_id| |k_jd|, w the true softmax, M_i = c2 max_j A_ij + 8 >= |m|.
    E_ij = (u + K_S U) c2 A_ij + K_S U M_i        the score's error in log2 units: the operand
           rounding bf16(fp32(c2 x)) is (1 + u)(1 + 2 U); the chain of 64 products onto -m is
           2 x 65 U (c2 A + |m|); the rescale's s - d one more of each: K_S = 2 x 65 + 4 = 134
    eta_ij = 2^E_ij (1 + u)(1 + 2 U) - 1          exp2 to 1 ulp, P rounded to bf16
    sigma_i = sum_j w_ij eta_ij                   asserted <= SIGMA_MAX = 1/2 (CPU and GPU)
  The bf16 terms are exact (2^E - 1, not E ln 2) and the weighted-mean perturbation below holds for
  every sigma < 1, so sigma only dilutes the check by 1 / (1 - sigma): SIGMA_MAX keeps that below 2.
  At u = 2^-8 the inputs give at most 0.034 (randn), 0.341 (3 randn), 0.141 (offset) and 0.138 (spike,
  selector: 2^(u c2 256) (1 + u) - 1).
  o    The kernel's o is the weighted mean of v with weights P^_j = c P_j (1 + e_j), |e_j| <= eta_j; a
       common factor c (the unknown m) cancels, so the check does not depend on the defer-max
       trajectory or the tile size:
           Bo_ic = [sum_j w_ij eta_ij |v_jc - o_ic| + K_O U sum_j w_ij (|v_jc| + |o_ic|)] / (1 - sigma_i)
           RNE(o - Bo) <= got <= RNE(o + Bo)
       K_O = 2 S + S / 64 + 3: the P.V chain of at most S products, the row sum l of at most S
       terms (fdot2, 2 each), one multiply per rescale on acc and l, rcp 2, the final multiply 1.
  lse  l 2^m = L (1 + sum w e): |got - lse| <= sigma / (1 - sigma) + K_L U (|lse| log2e + 1),
       K_L = 2 S + 4 S / 64 + 40: the row sum; per rescale alpha to 1 ulp, the multiply and m += d;
       log2 2 U log2 l with l <= 2^8 S (34); the sum m + log2 l; the constant ln 2 and its multiply.
  dQ   x_ij = 128 U c2 A_ij + 2 U |c2 s_ij| + 3 U |lq_i| (log2 units): the chain, the constant c2 and
       the fma's one rounding, lq's two and the fma's again; rP = 2^x (1 + 2 U) - 1.  G_ij =
       sum_c |dO_ic v_jc| (chain 128 U G), D_i = sum_c |dO_ic o_ic| (delta: 64 FMAs and the half-wave
       sum, 130 U D), the subtraction and the product U each:
           phi_ij = P_ij [(rP + 2 U) |dP_ij - delta_i| + (1 + rP)(128 U G_ij + 130 U D_i)]
           B_ic = scale sum_j (u |dS_ij| + (1 + u) phi_ij + (2 S + 1) U |dS_ij|) |k_jc|
           RNE(dQ - B) <= got <= RNE(dQ + B), and likewise dV and dK
  dV   E'_ij = (u + 2 U) c2 A_ij + 130 U (c2 A_ij + |lq_i|) + 3 U |lq_i| (the key prescaled, the chain
       of 65 onto -lq, lq itself):
           B_jc = sum_{i >= j} P_ij (2^E'_ij (1 + u)(1 + 2 U) - 1 + 2 S U) |dO_ic|
  dK   P stays fp32 in the product and dS is rounded once, so one factor 1 + u (not two):
           B_jc = scale sum_{i >= j} [|dS_ij| (2^E'_ij (1 + u)(1 + 3 U) - 1 + (2 S + 1) U)
                  + P_ij 2^E'_ij (1 + u)(130 U (G_ij + |delta_i|) + 130 U D_i)] |q_ic|
  Every bound carries FLOOR = 2^-100 absolute: a P below the fp32 normal range may be flushed.
  db   attn_bwd(..., with_bias_grad=True): the partials sum the unrounded fp32 accumulators, each
       within u (1 + 2 u) of its stored bf16 value, in fp32 (at most B S additions per column, 8 to
       spare for the butterfly and the LDS combine): each column must lie between the bf16 roundings
       of sum_rows dqkv_stored -+ (u (1 + 2 u) + (B S + 8) U) sum_rows |dqkv_stored| (db_bound's form).

Measured on an MI355X (each test prints its figures; 29 tests, 4.3 s, the slowest 0.8 s: the first, which
loads the extension).  A1: o and dV bit for bit at every shape and on the 2 GiB slices, lse at most
0.65 of 4 U ln n.  A2: no element other than the nearest bf16 value, band shares at most 0.39 %.  A3:
band shares 6.6 - 8.0 %, lse at 0.45 of its bound.  Family B, worst share of the bound that the output's
own rounding does not explain: o 0.09 - 0.12 (randn, 3 randn), 0.10 - 0.14 (spike), 0.01 (offset), 0.34
(selector); lse 0.08 - 0.36; dQ 0.26 - 0.85; dK 0.07 - 0.85; dV 0.13 - 0.81 (the largest of each on the
selector inputs, whose prescale rounding is systematic); db 0.09 - 0.17.  The CPU emulation of the
documented arithmetic gives the same figures to two digits, so the kernels round where this text says.
The bounds are worst case: on randn every rounding averages out and o uses a tenth of Bo, yet one
32-key block skipped for one wave's rows is 4.1 Bo (test_attention_exact_cpu.py).
"""
import functools
import math

import pytest
import torch

from test_gemm_dw_exact_gpu import check_bits, same_bits
from test_gemm_nt_exact_gpu import _quantum, as_bf16, rne
from test_ln_gelu_embed_gpu import check_banded, interval_ok, q16

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
D = 64
SCALE = 0.125
u = 2.0 ** -8
U = 2.0 ** -24
HO = 1.0 + 2.0 ** -10
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
C2 = float(torch.tensor(LOG2E, dtype=torch.float32)) / 8.0     # fp32(log2 e) / 8, exact
FLOOR = 2.0 ** -100
SHAPES = [(1, 128, 1), (2, 256, 3), (1, 512, 2)]
SHAPE_IDS = [f"B{b}-S{s}-H{h}" for b, s, h in SHAPES]
K_S = 2 * 65 + 4
SIGMA_MAX = 0.5
A2_CAP, A3_CAP = 0.02, 0.10       # largest share of elements whose band reaches a rounding midpoint
SEL_MATCH = 46.25                 # 16 bf16(16 c2) in log2 units
SEL_MIX_512 = (361, 88)           # rows that rescale, rows without a match at S = 512
BIG_S, BIG_H = 128, 43691         # S 3 H 64 2 B >= 2^31
KINDS = ("randn", "sharp", "spike", "offset", "selector")


def k_o(S):
    return 2 * S + S // 64 + 3


def k_l(S):
    return 2 * S + 4 * (S // 64) + 40


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def record(line):
    print(f"[attn-exact] {line}")


# ---------------------------------------------------------------------------------------------
# layouts: references hold [B, H, S, D] float64; the extension takes qkv [B, S, 3 H D], dO and o
# [B, S, H D] and returns lse [B, H, S]
# ---------------------------------------------------------------------------------------------
def pack_qkv(q, k, v):
    B, H, S, _ = q.shape
    x = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()     # [B, S, 3, H, D]
    return as_bf16(x).reshape(B, S, 3 * H * D)


def to_rows(t):
    """[B, H, S, D] float64 of bf16 values -> bf16 [B, S, H D]."""
    B, H, S, _ = t.shape
    return as_bf16(t.permute(0, 2, 1, 3).contiguous()).reshape(B, S, H * D)


def to_heads(t, H):
    """[B, S, H D] -> [B, H, S, D] (same dtype)."""
    B, S, _ = t.shape
    return t.reshape(B, S, H, D).permute(0, 2, 1, 3)


def split_dqkv(dqkv, H):
    """dqkv [B, S, 3 H D] -> dq, dk, dv as [B, H, S, D]."""
    B, S, _ = dqkv.shape
    x = dqkv.reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def flat2(t):
    """Any tensor as [rows, 64] for the bit checkers (CPU)."""
    return t.contiguous().reshape(-1, t.shape[-1]).cpu()


def tril(S, device):
    return torch.ones(S, S, dtype=torch.bool, device=device).tril()


def head_sig(B, H, device="cpu"):
    """[B, H, 1, 1] float64: 2^-((b H + h) mod 4)."""
    bh = torch.arange(B * H, device=device).reshape(B, H, 1, 1)
    return torch.exp2(-(bh % 4).to(F64))


def onehot_window(S, base, device="cpu"):
    """[S, 64] float64: row r = e_{r - base} for base <= r < base + 64, else 0."""
    t = torch.zeros(S, D, dtype=F64, device=device)
    i = torch.arange(64, device=device)
    t[base + i, i] = 1.0
    return t


def midpoint_share(v, band):
    """Share of elements whose band [v - band, v + band] reaches a bf16 rounding midpoint."""
    return float((rne(v - band) != rne(v + band)).double().mean())


def banded(got, v, band, what, cap):
    """check_banded on [rows, 64] views with the midpoint share capped."""
    share = midpoint_share(v, band)
    assert share <= cap, f"{what}: the band reaches a midpoint in {share:.3%} of the elements (cap {cap:.0%})"
    check_banded(flat2(got), flat2(v), flat2(band), what)
    return share


# ---------------------------------------------------------------------------------------------
# A1: uniform rows
# ---------------------------------------------------------------------------------------------
def recip_midpoint_distance(n):
    """Relative distance of 1 / n (float64 tensor n) from the nearest bf16 rounding midpoint."""
    x = 1.0 / n
    q = _quantum(x)
    mid = (torch.floor(x / q) + 0.5) * q
    return (x - mid).abs() / x


def a1_o_error(n):
    """Counted relative fp32 error of acc rcp(l): rcp to 1 ulp and one multiply."""
    return 3.0 * U * HO * torch.ones_like(n)


def a1_p_error(n):
    """Counted relative error of the dK / dV kernel's P~ = exp2(-fp32(lse log2e)) against 1 / n."""
    return (6.0 * torch.log(n) + 2.0) * U * HO


def a1_lse_expect(S, device="cpu"):
    n = torch.arange(1, S + 1, dtype=F64, device=device)
    return torch.log(n), 4.0 * U * HO * torch.log(n)


def a1_inputs(B, S, H, base, device="cpu"):
    z = torch.zeros(B, H, S, D, dtype=F64, device=device)
    return z, z, head_sig(B, H, device) * onehot_window(S, base, device)


def a1_o_expect(B, S, H, base, device="cpu"):
    """[B, H, S, D] bf16."""
    n = torch.arange(1, S + 1, dtype=F64, device=device)
    live = (base + torch.arange(D, device=device))[None, :] <= torch.arange(S, device=device)[:, None]
    e = torch.where(live, rne(1.0 / n)[:, None].expand(S, D), torch.zeros(S, D, dtype=F64, device=device))
    return as_bf16(head_sig(B, H, device) * e)


def a1_do(B, S, H, base, device="cpu"):
    return head_sig(B, H, device) * onehot_window(S, base, device)


def a1_dv_expect(B, S, H, base, device="cpu"):
    n = (base + torch.arange(D, device=device) + 1).to(F64)
    live = torch.arange(S, device=device)[:, None] <= (base + torch.arange(D, device=device))[None, :]
    e = torch.where(live, rne(1.0 / n)[None, :].expand(S, D), torch.zeros(S, D, dtype=F64, device=device))
    return as_bf16(head_sig(B, H, device) * e)


def check_a1_forward(o, lse, B, S, H, base, what):
    """o bf16 [B, H, S, D], lse fp32 [B, H, S]; returns the worst lse error / bound."""
    check_bits(flat2(o), flat2(a1_o_expect(B, S, H, base)), f"{what} o")
    ref, bound = a1_lse_expect(S)
    err = (lse.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), f"{what} lse: row {int((err > bound).nonzero()[0][-1])} off by " \
                                       f"{float(err.max()):.3e}"
    return float((err[..., 1:] / bound[1:]).max())


def check_a1_backward(dq, dk, dv, B, S, H, base, what):
    check_bits(flat2(dv), flat2(a1_dv_expect(B, S, H, base)), f"{what} dV")
    assert bool((dq == 0).all()) and bool((dk == 0).all()), f"{what}: dQ and dK must be exactly 0"


# ---------------------------------------------------------------------------------------------
# A2: dS structure
# ---------------------------------------------------------------------------------------------
def a2_pattern(B, S, H, device="cpu"):
    """[B, H, S] float64 in {0, 1}: a fixed random pattern per head; key 0 is set in every head."""
    g = torch.Generator().manual_seed(20240 + 7 * B + S + 13 * H)
    a = torch.randint(0, 2, (B, H, S), generator=g).to(F64)
    a[..., 0] = 1.0
    return a.to(device)


def a2_inputs(B, S, H, base, kind, device="cpu"):
    """q, k, v, dO [B, H, S, D]: kind 'dq' has K one-hot over the key window, 'dk' Q over the query window."""
    z = torch.zeros(B, H, S, D, dtype=F64, device=device)
    win = onehot_window(S, base, device).expand(B, H, S, D)
    v = z.clone()
    v[..., 0] = a2_pattern(B, S, H, device)
    do = z.clone()
    do[..., 0] = head_sig(B, H, device)[..., 0]
    return (z, win, v, do) if kind == "dq" else (win, z, v, do)


def a2_ds(B, S, H, o, lse):
    """The float64 dS [B, H, q, k] from the kernel's own o (bf16 [B, H, S, D]) and lse, and its band."""
    dev = o.device
    lse = lse.double()
    sig = head_sig(B, H, dev)[..., 0]                       # [B, H, 1]
    a = a2_pattern(B, S, H, dev)
    ds = torch.exp(-lse)[..., None] * sig[..., None] * (a[:, :, None, :] - o[..., 0].double()[..., None])
    ds = ds * tril(S, dev)
    return ds, (2.0 * lse.abs()[..., None] + 3.0) * U * HO * ds.abs()


def a2_dv_expect(B, S, H, device="cpu"):
    r = rne(1.0 / torch.arange(1, S + 1, dtype=F64, device=device))
    tail = torch.flip(torch.cumsum(torch.flip(r, [0]), 0), [0])      # sum_{q >= k} RNE(1 / (q + 1)): exact
    e = torch.zeros(B, H, S, D, dtype=F64, device=device)
    e[..., 0] = rne(head_sig(B, H, device)[..., 0] * tail)
    return as_bf16(e)


def check_a2(kind, base, o, lse, dq, dk, dv, B, S, H, what):
    """kind 'dq': dQ[q, c] = RNE(dS[q, base + c]) / 8, dK = 0; 'dk': dK[k, c] = RNE(dS[base + c, k]) / 8,
    dQ = 0; dV in both.  Returns the midpoint share."""
    ds, band = a2_ds(B, S, H, o, lse)
    if kind == "dq":
        share = banded(dq.double().mul(8.0).to(BF16), ds[..., base:base + 64], band[..., base:base + 64],
                       f"{what} dQ", A2_CAP)
        assert bool((dk == 0).all()), f"{what}: dK must be exactly 0"
    else:
        share = banded(dk.double().mul(8.0).to(BF16), ds[..., base:base + 64, :].transpose(-1, -2),
                       band[..., base:base + 64, :].transpose(-1, -2), f"{what} dK", A2_CAP)
        assert bool((dq == 0).all()), f"{what}: dQ must be exactly 0"
    check_bits(flat2(dv), flat2(a2_dv_expect(B, S, H)), f"{what} dV")
    return share


# ---------------------------------------------------------------------------------------------
# A3: selector rows
# ---------------------------------------------------------------------------------------------
def selector_maps(S):
    q = torch.arange(S)
    j = (7 * q + 3) % 64
    i = (5 * q + 11) % 64
    i[:70] = q[:70] % 8          # the first tile and six keys of the second use only dims 0 .. 7
    return j, i


def selector_mix(S):
    """(match [S, S] bool, rows that rescale, rows without a match)."""
    j, i = selector_maps(S)
    match = (j[:, None] == i[None, :]) & tril(S, "cpu")
    any_m = match.any(1)
    return match, int((any_m & ~match[:, :64].any(1)).sum()), int((~any_m).sum())


@functools.lru_cache(maxsize=None)
def selector_case(B, S, H):
    """q, k, v, dO [B, H, S, D] float64 (CPU)."""
    j, i = selector_maps(S)
    g = torch.Generator().manual_seed(4600 + 3 * B + S + 11 * H)
    q = torch.zeros(B, H, S, D, dtype=F64)
    k = torch.zeros(B, H, S, D, dtype=F64)
    q[:, :, torch.arange(S), j] = 16.0
    k[:, :, torch.arange(S), i] = 16.0
    v = head_sig(B, H) * torch.randint(-8, 9, (B, H, S, D), generator=g).to(F64)
    do = q16(torch.randn(B, H, S, D, generator=g))
    return q, k, v, do


def a3_expect(B, S, H, ref, v):
    """band of o, the expected lse [S] and its bound; ref = forward_reference(q, k, v) (CPU)."""
    match, _, _ = selector_mix(S)
    n = match.sum(1).to(F64)
    rows = torch.arange(1, S + 1, dtype=F64)
    lse = torch.where(n > 0, (SEL_MATCH + torch.log2(n.clamp_min(1.0))) * LN2, torch.log(rows))
    chain = 2.0 * 64.0 * (torch.arange(S, dtype=F64) // 64 + 1.0) + 3.0       # products in the row's tiles
    band = chain[:, None] * U * HO * (ref["w"] @ v.abs() + ref["o"].abs()) + 1e-10
    return band, lse, 5.0 * U * HO * lse.abs()


def check_a3(o, lse, ref, v, B, S, H, what):
    """o bf16 [B, H, S, D], lse fp32 [B, H, S], ref the float64 softmax of the selector case (CPU)."""
    band, want, bound = a3_expect(B, S, H, ref, v)
    share = banded(o, ref["o"], band, f"{what} o", A3_CAP)
    err = (lse.cpu().double() - want).abs()
    assert bool((err <= bound).all()), f"{what} lse: off by {float(err.max()):.3e}"
    return share, float((err / bound.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------
# family B: inputs, float64 references and counted bounds
# ---------------------------------------------------------------------------------------------
def spike_key(S):
    return S // 2 + 37      # mid-sequence, not on a tile edge


@functools.lru_cache(maxsize=None)
def b_case(kind, B, S, H):
    """q, k, v, dO [B, H, S, D] float64 of bf16 values (CPU); shared, never modified."""
    if kind == "selector":
        return selector_case(B, S, H)
    g = torch.Generator().manual_seed(977 * KINDS.index(kind) + 31 * B + S + 7 * H)
    r = lambda: torch.randn(B, H, S, D, generator=g)      # noqa: E731
    q, k, v, do = r(), r(), r(), r()
    if kind == "sharp":
        q, k = 3.0 * q, 3.0 * k
    elif kind == "spike":
        q[:] = 0.5
        k[:, :, spike_key(S)] = 8.0
    elif kind == "offset":
        q, k = 2.0 + 0.1 * q, 2.0 + 0.1 * k
    return q16(q), q16(k), q16(v), q16(do)


def forward_reference(q, k, v):
    """The float64 causal softmax attention of [B, H, S, D] inputs with the bounds of the docstring."""
    S, dev = q.shape[-2], q.device
    tri = tril(S, dev)
    s = (SCALE * (q @ k.transpose(-1, -2))).masked_fill(~tri, -math.inf)
    lse = torch.logsumexp(s, -1)
    w = torch.exp(s - lse[..., None])
    o = w @ v
    A = (q.abs() @ k.abs().transpose(-1, -2)) * tri
    Mi = C2 * A.amax(-1, keepdim=True) + 8.0
    E = (u + K_S * U) * C2 * A + K_S * U * Mi
    we = w * (torch.exp2(E) * (1.0 + u) * (1.0 + 2.0 * U) - 1.0)
    sigma = we.sum(-1)
    num = torch.empty_like(o)
    for c in range(0, D, 8):
        num[..., c:c + 8] = (we[..., None] * (v[..., None, :, c:c + 8] - o[..., :, None, c:c + 8]).abs()).sum(-2)
    Bo = (num + k_o(S) * U * HO * (w @ v.abs() + o.abs())) / (1.0 - sigma)[..., None] + FLOOR
    lse_bound = sigma / (1.0 - sigma) + k_l(S) * U * HO * (lse.abs() * LOG2E + 1.0)
    return dict(o=o, lse=lse, w=w, sigma=sigma, Bo=Bo, lse_bound=lse_bound)


def worst(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


def beyond_rounding(got, v):
    """Distance from the float64 v to the nearest real that RNE takes to the bf16 got: what the
    output's own rounding does not explain (printed as a share of the bound; the assertion itself is
    the interval rule)."""
    g = got.double()
    h = 0.5 * torch.where(g.abs() > v.abs(), _quantum(g * (1.0 - 2.0 ** -10)), _quantum(g))
    return ((g - v).abs() - h).clamp_min(0.0)


def check_rounded(got, v, bound, what):
    """The bf16 got is RNE of an fp32 value within `bound` of v: it lies between RNE(v - bound) and
    RNE(v + bound).  Returns the worst share of the bound in use."""
    assert got.dtype == BF16 and got.shape == v.shape, (what, got.dtype, got.shape)
    share = beyond_rounding(got, v) / bound
    ok = interval_ok(got.double(), v, bound)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside their interval, the worst at " \
                           f"{float(share[~ok].max()):.3f} of its bound at {_where(share * ~ok)}"
    return float(share.max())


def check_forward(ref, o, lse, what):
    """o bf16 [B, H, S, D], lse fp32 [B, H, S] on ref's device; returns the worst error / bound of each."""
    assert float(ref["sigma"].max()) <= SIGMA_MAX, f"{what}: sigma {float(ref['sigma'].max()):.3f} is outside the model"
    assert lse.dtype == torch.float32 and lse.shape == ref["lse"].shape
    el = (lse.double() - ref["lse"]).abs()
    rl = worst(el, ref["lse_bound"])
    record(f"{what}: worst error / bound: o {worst(beyond_rounding(o, ref['o']), ref['Bo']):.3f}, lse {rl:.3f} "
           f"(largest sigma {float(ref['sigma'].max()):.4f})")
    ro = check_rounded(o, ref["o"], ref["Bo"], f"{what} o")
    assert bool((el <= ref["lse_bound"]).all()), \
        f"{what}: lse at {rl:.3f} of its bound at {_where(el / ref['lse_bound'])}"
    return ro, rl


def _where(ratio):
    return tuple(int(x) for x in (ratio == ratio.max()).nonzero()[0])


def backward_reference(q, k, v, do, o, lse):
    """R2: float64 gradients from the kernel's own o (bf16 values) and lse, with the counted bounds.
    All [B, H, S, D] float64 but lse [B, H, S] float64."""
    S, dev = q.shape[-2], q.device
    tri = tril(S, dev)
    kt = k.transpose(-1, -2)
    s = SCALE * (q @ kt)
    P = torch.exp((s - lse[..., None]).masked_fill(~tri, -math.inf))
    dP = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1)[..., None]
    dS = P * (dP - delta)
    ref = dict(dq=SCALE * (dS @ k), dk=SCALE * (dS.transpose(-1, -2) @ q), dv=P.transpose(-1, -2) @ do)
    A = q.abs() @ k.abs().transpose(-1, -2)
    G = do.abs() @ v.abs().transpose(-1, -2)
    Dabs = (do * o).abs().sum(-1)[..., None]
    lq = lse.abs()[..., None] * LOG2E
    # dQ kernel
    x = 128.0 * U * C2 * A + 2.0 * U * s.abs() * LOG2E + 3.0 * U * lq
    rP = torch.exp2(x * HO) * (1.0 + 2.0 * U) - 1.0
    phi = P * ((rP + 2.0 * U) * (dP - delta).abs() + (1.0 + rP) * HO * (128.0 * U * G + 130.0 * U * Dabs))
    Mq = u * dS.abs() + (1.0 + u) * phi + (2 * S + 1) * U * HO * dS.abs()
    Bq = SCALE * (Mq @ k.abs()) + FLOOR
    # dK / dV kernel
    E2 = (u + 2.0 * U) * C2 * A + HO * (130.0 * U * (C2 * A + lq) + 3.0 * U * lq)
    gP = torch.exp2(E2)
    Bv = (P * (gP * (1.0 + u) * (1.0 + 2.0 * U) - 1.0 + 2 * S * U * HO)).transpose(-1, -2) @ do.abs() + FLOOR
    fdp = HO * (130.0 * U * (G + delta.abs()) + 130.0 * U * Dabs)
    Mk = dS.abs() * (gP * (1.0 + u) * (1.0 + 3.0 * U) - 1.0 + (2 * S + 1) * U * HO) + P * gP * (1.0 + u) * fdp
    Bk = SCALE * (Mk.transpose(-1, -2) @ q.abs()) + FLOOR
    ref.update(dq_bound=Bq, dk_bound=Bk, dv_bound=Bv)
    return ref


def check_backward(ref, dq, dk, dv, what):
    """dq, dk, dv bf16 [B, H, S, D]; returns the worst error / bound of each."""
    outs = (("dq", dq), ("dk", dk), ("dv", dv))
    record(f"{what}: worst error / bound: " +
           ", ".join(f"{n} {worst(beyond_rounding(g, ref[n]), ref[n + '_bound']):.3f}" for n, g in outs))
    return {n: check_rounded(g, ref[n], ref[n + "_bound"], f"{what} {n}") for n, g in outs}


def db_interval(stored, rows):
    """Column sums of the stored dqkv [rows, 3 H D] (float64) and the bound of the docstring."""
    return stored.sum(0), (u * (1.0 + 2.0 * u) + (rows + 8) * U * HO) * stored.abs().sum(0)


def check_db(db, dqkv, what):
    """db bf16 [3 H D] against the stored dqkv [B, S, 3 H D]; returns what the bound explains."""
    rows = dqkv.shape[0] * dqkv.shape[1]
    s, bound = db_interval(dqkv.reshape(rows, -1).double(), rows)
    got = db.double()
    bad = ~interval_ok(got, s, bound)
    assert not bool(bad.any()), f"{what}: column {int(bad.nonzero()[0])} of db outside its interval"
    return float((((got - s).abs() - 0.5 * _quantum(s)).clamp_min(0.0) / bound.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
def run_forward(m, q, k, v):
    """[B, H, S, D] float64 on the GPU -> qkv, o (rows), lse, o as heads."""
    H = q.shape[1]
    qkv = pack_qkv(q, k, v)
    o, lse = m.attn_fwd(qkv, H)
    return qkv, o, lse, to_heads(o, H)


def run_backward(m, qkv, o, lse, do, H, **kw):
    outs = m.attn_bwd(to_rows(do), qkv, o, lse, H, **kw)
    return split_dqkv(outs[0], H), outs


@pytest.mark.parametrize("B,S,H", SHAPES, ids=SHAPE_IDS)
def test_a1_uniform_rows(cuda, B, S, H):
    """A1: o bit for bit over the whole triangle and +0 above it, lse = ln(q + 1) within 4 U ln n,
    dV bit for bit, dQ = dK = 0."""
    m = _m()
    rl = 0.0
    for base in range(0, S, 64):
        q, k, v = a1_inputs(B, S, H, base, cuda)
        _, _, lse, oh = run_forward(m, q, k, v)
        rl = max(rl, check_a1_forward(oh, lse, B, S, H, base, f"A1 {B}x{S}x{H} window {base}"))
    z = torch.zeros(B, H, S, D, dtype=F64, device=cuda)
    qkv, o, lse, _ = run_forward(m, z, z, z)
    for base in range(0, S, 64):
        (dq, dk, dv), _ = run_backward(m, qkv, o, lse, a1_do(B, S, H, base, cuda), H)
        check_a1_backward(dq, dk, dv, B, S, H, base, f"A1 {B}x{S}x{H} query window {base}")
    record(f"A1 {B}x{S}x{H}: o and dV bit for bit; worst lse error / bound {rl:.3f}")


@pytest.mark.parametrize("B,S,H", SHAPES, ids=SHAPE_IDS)
def test_a2_ds_structure(cuda, B, S, H):
    """A2: dQ and dK are single rounded dS values under the band rule, from the kernel's own o and lse."""
    m = _m()
    shares = []
    for kind in ("dq", "dk"):
        for base in range(0, S, 64):
            q, k, v, do = a2_inputs(B, S, H, base, kind, cuda)
            qkv, o, lse, oh = run_forward(m, q, k, v)
            (dq, dk, dv), _ = run_backward(m, qkv, o, lse, do, H)
            shares.append(check_a2(kind, base, oh.cpu(), lse.cpu(), dq.cpu(), dk.cpu(), dv.cpu(), B, S, H,
                                   f"A2 {B}x{S}x{H} {kind} window {base}"))
    record(f"A2 {B}x{S}x{H}: largest midpoint share {max(shares):.3%} (cap {A2_CAP:.0%})")


@pytest.mark.parametrize("B,S,H", SHAPES, ids=SHAPE_IDS)
def test_a3_selector_rows(cuda, B, S, H):
    """A3: the score path through every head-dim index and the rescale by 2^-46.25."""
    m = _m()
    _, resc, nomatch = selector_mix(S)
    assert resc > 0 and nomatch > 0 and (S != 512 or (resc, nomatch) == SEL_MIX_512)
    q, k, v, _ = (t.to(cuda) for t in selector_case(B, S, H))
    _, _, lse, oh = run_forward(m, q, k, v)
    ref = {n: x.cpu() for n, x in forward_reference(q, k, v).items()}
    share, rl = check_a3(oh.cpu(), lse.cpu(), ref, v.cpu(), B, S, H, f"A3 {B}x{S}x{H}")
    record(f"A3 {B}x{S}x{H}: {resc} rows rescale, {nomatch} without a match; midpoint share {share:.3%} "
           f"(cap {A3_CAP:.0%}); worst lse error / bound {rl:.3f}")


@pytest.mark.parametrize("B,S,H", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_b_per_element_fp64(cuda, kind, B, S, H):
    """Family B: o and lse against the true softmax, dQ / dK / dV against the R2 formula from the
    kernel's own o and lse, every element within its counted bound."""
    m = _m()
    q, k, v, do = (t.to(cuda) for t in b_case(kind, B, S, H))
    qkv, o, lse, oh = run_forward(m, q, k, v)
    what = f"B {kind} {B}x{S}x{H}"
    check_forward(forward_reference(q, k, v), oh, lse, what)
    (dq, dk, dv), _ = run_backward(m, qkv, o, lse, do, H)
    check_backward(backward_reference(q, k, v, do, oh.double(), lse.double()), dq, dk, dv, what)


@pytest.mark.parametrize("B,S,H", SHAPES, ids=SHAPE_IDS)
def test_fused_bias_gradient(cuda, B, S, H):
    """db of attn_bwd(with_bias_grad=True) per column inside the interval of the docstring; dqkv is
    that of the plain call, bit for bit."""
    m = _m()
    q, k, v, do = (t.to(cuda) for t in b_case("randn", B, S, H))
    qkv, o, lse, _ = run_forward(m, q, k, v)
    _, plain = run_backward(m, qkv, o, lse, do, H)
    _, outs = run_backward(m, qkv, o, lse, do, H, with_bias_grad=True)
    assert len(outs) == 2 and outs[1].shape == (3 * H * D,) and outs[1].dtype == BF16
    assert same_bits(outs[0], plain[0])
    r = check_db(outs[1], outs[0], f"db {B}x{S}x{H}")
    record(f"db {B}x{S}x{H}: worst (|db - sum| - half a bf16 spacing) / bound {r:.3f}")


def test_rejections(cuda):
    """S = 192 and head dim 32 raise before any launch; a valid call follows each."""
    m = _m()

    def good():
        q, k, v = a1_inputs(1, 128, 1, 0, cuda)
        _, _, lse, oh = run_forward(m, q, k, v)
        check_a1_forward(oh, lse, 1, 128, 1, 0, "A1 after a rejection")

    for S, H, width in ((192, 1, 64), (128, 2, 32)):
        qkv = torch.zeros(1, S, 3 * H * width, dtype=BF16, device=cuda)
        o = torch.zeros(1, S, H * width, dtype=BF16, device=cuda)
        lse = torch.zeros(1, H, S, dtype=torch.float32, device=cuda)
        with pytest.raises(RuntimeError):
            m.attn_fwd(qkv, H)
        with pytest.raises(RuntimeError):
            m.attn_bwd(o, qkv, o, lse, H)
        good()


def test_slices_of_2_gib(cuda):
    """S 3 H 64 2 B >= 2^31: the pointer-staging attn_fwd3_d64<0> and attn_bwd_dq_d64<0> run.  A1 (o,
    lse, dV) and A2 (dQ) on heads 0, 1, H / 2 and H - 1, the references for those heads only.  One
    qkv (2 GiB), o and dO (0.7 GiB each), dqkv (2 GiB) and the workspace are alive at once, about
    6 GiB at the peak, freed before the next window."""
    m = _m()
    S, H = BIG_S, BIG_H
    assert S * 3 * H * D * 2 >= 1 << 31
    heads = torch.tensor([0, 1, H // 2, H - 1], device=cuda)
    sig = torch.exp2(-(torch.arange(H, device=cuda) % 4).to(F64)).to(BF16)       # 2^-(h mod 4), B = 1
    sig4 = sig[heads].double()[None, :, None, None]                              # [1, 4, 1, 1]
    a = a2_pattern(1, S, 1, cuda)[0, 0]                                          # one pattern for every head
    rl = 0.0

    def pick(t):     # [1, S, H D] -> [1, 4, S, D] on the chosen heads
        return t.view(S, H, D)[:, heads].permute(1, 0, 2)[None]

    for base in range(0, S, 64):
        win = onehot_window(S, base, cuda).to(BF16)
        # A1 forward
        qkv = torch.zeros(1, S, 3, H, D, device=cuda, dtype=BF16)
        qkv[0, :, 2] = win[:, None, :] * sig[None, :, None]
        o, lse = m.attn_fwd(qkv.view(1, S, 3 * H * D), H)
        want = as_bf16(sig4.cpu() * a1_o_expect(1, S, 1, base).double())
        check_bits(flat2(pick(o)), flat2(want), f"2 GiB A1 o window {base}")
        ref, bound = a1_lse_expect(S)
        err = (lse.view(H, S)[heads].cpu().double() - ref).abs()
        assert bool((err <= bound).all()), f"2 GiB A1 lse window {base}: off by {float(err.max()):.3e}"
        rl = max(rl, float((err[:, 1:] / bound[1:]).max()))
        # A1 backward: Q = K = V = 0, dO the window
        qkv.zero_()
        qkv = qkv.view(1, S, 3 * H * D)
        o, lse = m.attn_fwd(qkv, H)
        do = (win[:, None, :] * sig[None, :, None]).reshape(1, S, H * D)
        dqkv = m.attn_bwd(do, qkv, o, lse, H)[0].view(S, 3, H, D)
        want = as_bf16(sig4.cpu() * a1_dv_expect(1, S, 1, base).double())
        check_bits(flat2(dqkv[:, 2][:, heads].permute(1, 0, 2)), flat2(want[0]), f"2 GiB A1 dV window {base}")
        assert bool((dqkv[:, :2][:, :, heads] == 0).all()), "2 GiB A1: dQ and dK must be exactly 0"
        del dqkv, do
        # A2 dQ: Q = 0, K the window, V = a_k e_0, dO = sig e_0
        qkv = qkv.view(1, S, 3, H, D)
        qkv[0, :, 1] = win[:, None, :]
        qkv[0, :, 2, :, 0] = a.to(BF16)[:, None]
        qkv = qkv.view(1, S, 3 * H * D)
        o, lse = m.attn_fwd(qkv, H)
        do = torch.zeros(S, H, D, device=cuda, dtype=BF16)
        do[:, :, 0] = sig[None, :]
        dqkv = m.attn_bwd(do.view(1, S, H * D), qkv, o, lse, H)[0].view(S, 3, H, D)
        o4, l4 = pick(o).cpu().double(), lse.view(H, S)[heads].cpu().double()[None]      # [1, 4, S, D], [1, 4, S]
        ds = torch.exp(-l4)[..., None] * sig4.cpu() * (a.cpu()[None, None, None, :] - o4[..., :1]) * tril(S, "cpu")
        band = (2.0 * l4.abs()[..., None] + 3.0) * U * HO * ds.abs()
        dq = dqkv[:, 0][:, heads].permute(1, 0, 2)[None].cpu()
        banded(dq.double().mul(8.0).to(BF16), ds[..., base:base + 64], band[..., base:base + 64],
               f"2 GiB A2 dQ window {base}", A2_CAP)
        del qkv, o, lse, do, dqkv
    record(f"2 GiB slices: A1 o, dV bit for bit and A2 dQ banded on heads {heads.tolist()}; worst lse error / bound "
           f"{rl:.3f}")
