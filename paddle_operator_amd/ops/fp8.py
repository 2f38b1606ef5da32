"""FP8 (OCP e4m3) forward products: per-tensor power-of-two quantisation and
the e4m3 GEMM (csrc/hip/quant_f8.hip, csrc/hip/gemm_nt_f8.hip).

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


def _f8_ok(x, w, b) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.is_contiguous()
            and w.is_contiguous() and w.dim() == 2 and (b is None or b.dtype == torch.bfloat16)
            and _native.require_hip().gemm_nt_f8_supported(x.numel() // x.shape[-1], w.shape[0], w.shape[1]))


def _fwd_gemm_f8(x, w, b=None):
    """x·Wᵀ (+ b) with both operands quantised to e4m3 just in time: two quantiser launches per operand, then
    gemm_nt_f8 with the bias in its epilogue.  Outside its shape contract: ``_fwd_gemm``, the bf16 product."""
    if not _f8_ok(x, w, b):
        return _fwd_gemm(x, w, b)
    m = _native.require_hip()
    qx, dx = m.quant_e4m3(x.reshape(-1, x.shape[-1]))
    qw, dw = m.quant_e4m3(w)
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
