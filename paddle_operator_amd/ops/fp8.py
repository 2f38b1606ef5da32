"""FP8 (OCP e4m3) forward products: per-tensor power-of-two quantisation and
the e4m3 GEMMs (csrc/hip/quant_f8.hip, csrc/hip/gemm_nt_f8.hip, csrc/hip/gemm_nt_mx8.hip).

Straight-through FP8 forward training: only the forward product y = x·Wᵀ (+ b)
runs on e4m3 operands; the backward keeps the saved **bf16** x and W and is
``ops.linear``'s, gradient for gradient.  The scale is computed just in time
from the tensor's own max |x| — no scaling state, so checkpoints and exact
resume are untouched.

Scale rule (the kernels' and ``ref_quant_e4m3``'s, from the bits of amax =
m·2^a, m ∈ [1, 2)): s = 2^e with e = 8 − a for m ≤ 1.75, else 7 − a, so that
amax·s ∈ (224, 448] (448 = e4m3's largest finite value); amax = 0 → e = 0;
|e| ≤ 126 keeps s and 1/s normal.  q = RNE_e4m3(x·s); the GEMM multiplies the
fp32 sums by 2^−e of both operands.

Two forms of the activation operand:

* per tensor, just in time (``linear_fp8``, ``GPT2Config.fp8 = "qkv"``): an amax
  pass and a convert pass over x in front of the GEMM;
* per token, from the producer (``linear_fp8_rows``, ``GPT2Config.fp8 = "ln"``):
  the LayerNorm that computes x also writes each row as e4m3 under the row's
  own scale — the rule above with amax taken over one row of the bf16-rounded
  output (``ref_quant_e4m3_rows``) — and hands (q, 2^−e per row) to the GEMM,
  which multiplies each output row by its token's scale in the epilogue.  No
  pass over x, at least as fine a scale, still no state.

A third form, for an operand whose producer never sees a whole row:

* per (token, 32 columns): rows as MXFP8 — e4m3 bytes and one E8M0 scale byte per 32 consecutive columns, the rule
  above with amax taken over the block of the bf16-rounded values (``ref_quant_mx8_rows``; not the OCP floor rule,
  which lets amax·2^e reach 512 and saturates); the byte is 127 − e, the E8M0 code of 2^−e, the form gfx950's
  scaled MFMA takes per 32 k (``ref_linear_mx8_rows``).  This is fc2 under ``GPT2Config.fp8 = "lnmx"``: fc1's GELU
  epilogue on gemm_nt_f8 writes its bf16 output once more as such rows (``gemm_nt_f8_gelu(mx=True)``, bit for bit
  ``ref_quant_mx8_rows`` of the stored bf16), and ``gemm_nt_mx8`` multiplies them with the per-tensor e4m3 W2 on
  the scaled MFMA, adding fc2's bias and the residual stream in its epilogue (``ops.mlp(mx=True)``,
  ``ops.mlp_add_layer_norm(mx=True)``).  The bf16 output is still stored: the backward and fc2's dW read it.

The weight is quantised per tensor in all three: once per optimizer step for the weights a trainer registered
(``parallel.flat.FlatParams.enable_wq``: one grouped launch pair when ``wt_scope`` opens, the e4m3 bytes and scale
read from the arena while it is live), just in time per call everywhere else — the same bytes (``_weight_e4m3``).
"""
from __future__ import annotations

import torch

from .. import _native
from .core import _LinearFn, _fwd_gemm, linear, use_hip


def _scale_exp(amax_bits: int) -> int:
    if amax_bits == 0:
        return 0
    a = (amax_bits >> 23) - 127
    e = (8 if (amax_bits & 0x7FFFFF) <= 0x600000 else 7) - a
    return max(-126, min(126, e))


def ref_quant_e4m3(x: torch.Tensor):
    """(e4m3 bytes shaped like x, 2^−e as a float32[1]) by the rule above, in
    plain torch on the CPU; finite inputs only."""
    xf = x.detach().float().cpu()
    amax = xf.abs().max().reshape(1) if xf.numel() else torch.zeros(1)
    e = _scale_exp(int(amax.view(torch.int32)) & 0x7FFFFFFF)
    q = (xf * (2.0 ** e)).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.to(x.device), torch.tensor([2.0 ** -e], dtype=torch.float32, device=x.device)


def _dequant(q: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    return q.cpu().view(torch.float8_e4m3fn).float() * d.cpu()


def ref_linear_fp8(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None = None) -> torch.Tensor:
    """The e4m3 product in plain torch: dequantised operands, fp32 product (+ b), one rounding to x's dtype."""
    y = _dequant(*ref_quant_e4m3(x)) @ _dequant(*ref_quant_e4m3(w)).t()
    if b is not None:
        y = y + b.detach().float().cpu()
    return y.to(x.dtype).to(x.device)


# the e4m3 weights of a trainer's step taken from the arena (FlatParams.enable_wq) instead of quantised per call; read
# when wt_scope opens.  Same bits either way (tests/test_fp8_wq_gpu.py); measured in profiles/fp8_wq.md
_WQ_ARENA = [True]


def _live_wq(w):
    """The arena's e4m3 copy (q, 2^−e) of ``w`` (parallel.flat.FlatParams.enable_wq) while it is live (inside the
    trainer's wt_scope), else None."""
    t = getattr(w, "_pdo_wq", None)
    if t is not None and t[0].wq_live:
        return t[1], t[2]
    return None


def _weight_e4m3(w):
    """(q, 2^−e) of the weight ``w``: the step's arena copy while live, else quantised just in time."""
    return _live_wq(w) or _native.require_hip().quant_e4m3(w)


def _f8_ok(x, w, b) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.is_contiguous()
            and w.is_contiguous() and w.dim() == 2 and (b is None or b.dtype == torch.bfloat16)
            and _native.require_hip().gemm_nt_f8_supported(x.numel() // x.shape[-1], w.shape[0], w.shape[1]))


def _fwd_gemm_f8(x, w, b=None):
    """x·Wᵀ (+ b) with both operands as e4m3: x quantised just in time (two quantiser launches), W by
    ``_weight_e4m3``, then gemm_nt_f8 with the bias in its epilogue.  Outside its shape contract: ``_fwd_gemm``, the bf16 product."""
    if not _f8_ok(x, w, b):
        return _fwd_gemm(x, w, b)
    m = _native.require_hip()
    qx, dx = m.quant_e4m3(x.reshape(-1, x.shape[-1]))
    qw, dw = _weight_e4m3(w)
    return m.gemm_nt_f8(qx, dx, qw, dw, b).view(*x.shape[:-1], w.shape[0])


class _LinearF8Fn(_LinearFn):
    """``_LinearFn`` with the forward product on e4m3 operands (HIP) or as ``ref_linear_fp8`` (elsewhere); the
    saved tensors are the bf16 x and W and the backward is ``_LinearFn``'s, inherited."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        ctx.b = b
        return _fwd_gemm_f8(x, w, b) if use_hip(x) else ref_linear_fp8(x, w, b)


def linear_fp8(x, w, b=None):
    """y = x·Wᵀ (+ b) with an FP8 forward product and ``ops.linear``'s bf16 backward; ``ops.linear`` itself where
    the e4m3 GEMM does not take the shape."""
    if use_hip(x) and not _f8_ok(x, w, b):
        return linear(x, w, b)
    return _LinearF8Fn.apply(x, w, b)


# ----------------------------------------------------------------------------
# per-token scales: the A operand as e4m3 rows written by the producing LayerNorm
# (``GPT2Config.fp8 = "ln"``; csrc/hip/layernorm.hip Q8, gemm_nt_f8's row form)
# ----------------------------------------------------------------------------

def ref_quant_e4m3_rows(y: torch.Tensor):
    """``ref_quant_e4m3`` applied to each row of y [..., C] on its own, in plain torch on the CPU:
    (e4m3 bytes [rows, C], 2^−e per row as float32 [rows])."""
    yf = y.detach().float().cpu().reshape(-1, y.shape[-1])
    bits = yf.abs().amax(dim=1).view(torch.int32) & 0x7FFFFFFF
    e = torch.where((bits & 0x7FFFFF) <= 0x600000, 8, 7) - ((bits >> 23) - 127)
    e = torch.where(bits == 0, 0, e.clamp(-126, 126))
    one = torch.ones(e.shape, dtype=torch.float32)
    q = (yf * torch.ldexp(one, e).unsqueeze(1)).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.to(y.device), torch.ldexp(one, -e).to(y.device)


def ln_q8_ok(h: torch.Tensor, *weights) -> bool:
    """Whether the LayerNorm that produces h [..., C] should also write e4m3 rows for the products h·Wᵀ of
    ``weights``: each within gemm_nt_f8's contract on the HIP path; always off it (the plain-torch reference)."""
    if not use_hip(h):
        return True
    T = h.numel() // h.shape[-1]
    m = _native.require_hip()
    return h.dtype == torch.bfloat16 and all(
        w.dtype == torch.bfloat16 and w.dim() == 2 and w.is_contiguous() and w.shape[1] == h.shape[-1]
        and m.gemm_nt_f8_supported(T, w.shape[0], w.shape[1]) for w in weights)


def _rows_ok(q, d, w, b=None) -> bool:
    return (q is not None and q.is_cuda and w.dtype == torch.bfloat16 and w.dim() == 2 and w.is_contiguous()
            and (b is None or b.dtype == torch.bfloat16) and q.shape[-1] == w.shape[1] and d.numel() == q.shape[0]
            and _native.require_hip().gemm_nt_f8_supported(q.shape[0], w.shape[0], w.shape[1]))


def _fwd_gemm_f8_rows(q, d, w, b=None):
    """[rows, N] = (q·Wᵀ)·d[row]·dw (+ b): q, d the LayerNorm's rows and per-token scales, W quantised per
    tensor (``_weight_e4m3``) as ``_fwd_gemm_f8`` does; the caller has checked ``_rows_ok``."""
    m = _native.require_hip()
    qw, dw = _weight_e4m3(w)
    return m.gemm_nt_f8(q, d, qw, dw, b)


def ref_linear_fp8_rows(q, d, w, b=None, dtype=torch.bfloat16):
    """The per-token-scaled e4m3 product in plain torch: dequantised rows · dequantised W in fp32 (+ b), one rounding."""
    a = q.cpu().view(torch.float8_e4m3fn).float() * d.cpu().float().unsqueeze(1)
    y = a @ _dequant(*ref_quant_e4m3(w)).t()
    if b is not None:
        y = y + b.detach().float().cpu()
    return y.to(dtype).to(q.device)


class _LinearF8RowsFn(_LinearFn):
    """``_LinearFn`` whose forward product takes x as the e4m3 rows (q, d) its LayerNorm wrote; saves the bf16
    x and W, and the backward is ``_LinearFn``'s."""

    @staticmethod
    def forward(ctx, x, w, b, q, d):
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        ctx.b = b
        if use_hip(x):
            return _fwd_gemm_f8_rows(q, d, w, b).view(*x.shape[:-1], w.shape[0])
        return ref_linear_fp8_rows(q, d, w, b, x.dtype).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        return _LinearFn.backward(ctx, dy) + (None, None)


def linear_fp8_rows(x, f8, w, b=None):
    """y = x·Wᵀ (+ b) with the forward product on ``f8`` = (q, d), x's e4m3 rows and per-token scales, and
    ``ops.linear``'s bf16 backward; ``ops.linear`` itself where the e4m3 GEMM does not take the shape."""
    if use_hip(x) and not _rows_ok(f8[0], f8[1], w, b):
        return linear(x, w, b)
    return _LinearF8RowsFn.apply(x, w, b, f8[0], f8[1])


# ----------------------------------------------------------------------------
# MXFP8 rows: one E8M0 scale per (token, 32 columns), written by fc1's epilogue and read by gemm_nt_mx8
# (``GPT2Config.fp8 = "lnmx"``; csrc/hip/gemm_nt_f8.hip MX, csrc/hip/gemm_nt_mx8.hip)
# ----------------------------------------------------------------------------

def ref_quant_mx8_rows(y: torch.Tensor):
    """``ref_quant_e4m3`` applied to each block of 32 consecutive columns of each row of y [..., K], K % 32 = 0, in
    plain torch on the CPU: (e4m3 bytes uint8 [rows, K], E8M0 scale bytes uint8 [rows, K / 32] = 127 − e)."""
    K = y.shape[-1]
    yf = y.detach().float().cpu().reshape(-1, K // 32, 32)
    bits = yf.abs().amax(dim=2).view(torch.int32) & 0x7FFFFFFF
    e = torch.where((bits & 0x7FFFFF) <= 0x600000, 8, 7) - ((bits >> 23) - 127)
    e = torch.where(bits == 0, 0, e.clamp(-126, 126))
    q = (yf * torch.ldexp(torch.ones(e.shape), e).unsqueeze(2)).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.reshape(-1, K).to(y.device), (127 - e).to(torch.uint8).to(y.device)


def ref_linear_mx8_rows(q, s, w, b=None, res=None, dtype=torch.bfloat16):
    """The MXFP8 product in plain torch: rows dequantised block by block (q·2^(s − 127)) · dequantised W in fp32
    (+ b) (+ res), one rounding.  W is quantised per tensor (``ref_quant_e4m3``)."""
    d = torch.ldexp(torch.ones(s.shape), s.cpu().to(torch.int32) - 127)
    a = q.cpu().view(torch.float8_e4m3fn).float() * d.repeat_interleave(32, dim=1)
    y = a @ _dequant(*ref_quant_e4m3(w)).t()
    if b is not None:
        y = y + b.detach().float().cpu()
    if res is not None:
        y = y + res.detach().float().cpu().reshape(y.shape)
    return y.to(dtype).to(q.device)


def _mx_ok(T, w, b=None, res=None) -> bool:
    """Whether gemm_nt_mx8 takes [T, K] MXFP8 rows · Wᵀ (+ b + res): W bf16 contiguous [N, K] within the kernel's
    shape contract, res (which comes with b) bf16 contiguous of T·N elements."""
    return (w.is_cuda and w.dtype == torch.bfloat16 and w.dim() == 2 and w.is_contiguous()
            and (b is None or b.dtype == torch.bfloat16)
            and (res is None or (b is not None and res.dtype == torch.bfloat16 and res.is_contiguous()
                                 and res.numel() == T * w.shape[0]))
            and _native.require_hip().gemm_nt_mx8_supported(T, w.shape[0], w.shape[1]))


def _fwd_gemm_mx8(q, s, w, b=None, res=None):
    """[rows, N] = (q·2^(s − 127))·Wᵀ·dw (+ b) (+ res): q, s the MXFP8 rows fc1's epilogue wrote, W quantised per
    tensor just in time as ``_fwd_gemm_f8_rows`` does; the caller has checked ``_mx_ok``."""
    m = _native.require_hip()
    qw, dw = _weight_e4m3(w)
    return m.gemm_nt_mx8(q, s, qw, dw, b, None if res is None else res.reshape(-1, w.shape[0]))
