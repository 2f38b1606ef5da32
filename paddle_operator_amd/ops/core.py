"""Shared machinery of the HIP op bindings (``ops.gpt2``, ``ops.resnet``).

* device dispatch (``use_hip``): a GPU tensor runs the HIP kernel in
  ``csrc/hip`` — a missing extension raises, never a silent fallback;
* plain PyTorch fp32 references (``ref_*``): the CPU path and the numerics
  tests' oracle (``tests/test_ops_gpu.py``);
* the flat-arena gradient hand-off: weight / bias / norm-weight gradients
  written or reduced straight into the parameter's arena slice
  (``_arena_grads``, ``_signal_ready``), deferred batched column sums
  (``deferred_reductions``), weight-gradient GEMMs grouped into whole rounds
  (``deferred_weight_grads``), the step's prebuilt Wᵀ operands (``transpose``);
* ``linear`` on gemm_nt4 (forward, dX) and gemm_dw4 (dW into the arena).

The module-level one-element lists (``_NT_ALL``, ``_HIP_DW``, …) are test
hooks that switch a fused path off for an on/off comparison; they are not
user knobs (round 5 retired the ``PDO_*`` environment switches that set them).
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

from .. import _native


def use_hip(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    if _native.ops_mode() == "torch":
        return False
    _native.require_hip()
    return True

# ----------------------------------------------------------------------------
# reference implementations (fp32 math, cast back to input dtype)
# ----------------------------------------------------------------------------

def ref_layer_norm(x, w, b, eps=1e-5):
    y = F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps)
    return y.to(x.dtype)


def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))


def ref_bias_gelu(x, b):
    return _gelu_tanh(x.float() + b.float()).to(x.dtype)


def ref_attention(q, k, v, causal=True, keep=None, scale=1.0, math_dtype=torch.float32):
    """q,k,v: [B, H, S, D] → [B, H, S, D] (fp32 math).

    ``keep`` (bool [B, H, S, S], ``philox_attn_keep_mask``) and ``scale``:
    attention-probability dropout with an explicit mask — the softmax is taken
    over the undropped scores, then P ← keep ? P·scale : 0.  Differentiable.
    ``math_dtype``: the dtype of the two matmuls' operands (the softmax stays
    fp32); bf16 makes this the framework-bf16 form of the same computation."""
    qf, kf, vf = q.to(math_dtype), k.to(math_dtype), v.to(math_dtype)
    s = (qf @ kf.transpose(-1, -2)).float() / math.sqrt(q.shape[-1])
    if causal:
        S = q.shape[-2]
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = torch.where(keep.to(p.device), p * scale, torch.zeros((), dtype=p.dtype, device=p.device))
    return (p.to(math_dtype) @ vf).to(q.dtype)


def ref_cross_entropy(logits, target, vocab: int | None = None):
    """Mean token cross entropy; columns >= ``vocab`` (padding) are masked."""
    lf = logits.float()
    if vocab is not None and vocab < lf.shape[-1]:
        lf = lf[..., :vocab]
    return F.cross_entropy(lf.reshape(-1, lf.shape[-1]), target.reshape(-1))


# ----------------------------------------------------------------------------
# counter-based dropout masks (host reference of csrc/hip/philox.h)
# ----------------------------------------------------------------------------

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 in numpy ``uint64`` arithmetic: ``counter`` = four arrays
    (or ints) of 32-bit words, ``key`` = two 32-bit ints; returns the four output
    word arrays (uint64 holding 32-bit values)."""
    import numpy as np
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(_U32) for c in counter)
    k0, k1 = int(key[0]) & _U32, int(key[1]) & _U32
    m0, m1, mask, sh = np.uint64(_PHILOX_M0), np.uint64(_PHILOX_M1), np.uint64(_U32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 × 32 → 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + _PHILOX_W0) & _U32, (k1 + _PHILOX_W1) & _U32
    return c0, c1, c2, c3


def philox_keep_mask(shape, thr: int, seed: int, site: int, step: int, offset: int = 0) -> torch.Tensor:
    """The dropout keep mask of a ``[..., C]`` tensor (C % 8 == 0) as the HIP
    kernels draw it (csrc/hip/philox.h), built on the host: a bool tensor, True =
    kept.  One Philox4x32-10 call per group of 8 consecutive elements; key =
    (low, high) half of the 64-bit ``seed``; counter = (g_lo, g_hi, site, step)
    with g = ``offset`` + the group's index in the flattened tensor; element j
    takes output word j >> 1, bits 0-15 (j even) or 16-31 (j odd), and is kept
    iff that value ≥ ``thr`` = round(p·65536).

    This backs the CPU path of every op that takes ``drop`` and the GPU
    ``PDO_OPS=torch`` path (mask built here and copied: a parity path, not a fast
    one), so a CPU fp32 model and the HIP bf16 model drop the same elements."""
    import numpy as np
    shape = tuple(shape)
    n = int(np.prod(shape, dtype=np.int64))
    if not shape or shape[-1] % 8 or not 0 <= thr <= 65535:
        raise ValueError(f"philox_keep_mask: last dim % 8 and thr in [0, 65535] required, got {shape}, {thr}")
    g = (np.arange(n // 8, dtype=np.uint64) + np.uint64(offset & 0xFFFFFFFFFFFFFFFF))  # wraps mod 2^64
    words = philox4x32_10((g & np.uint64(_U32), g >> np.uint64(32), site, step), (seed & _U32, (seed >> 32) & _U32))
    w = np.stack(words, axis=1)  # [groups, 4]
    v = np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=2).reshape(-1, 8)  # element j: word j>>1, half j&1
    return torch.from_numpy(v >= np.uint64(thr)).reshape(shape)


class Dropout(tuple):
    """(thr, scale, seed, site, step): one dropout site of one training step.
    ``thr`` = round(p·65536) (p is quantised to 1/65536), ``scale`` =
    65536 / (65536 − thr) in fp32, ``seed`` the 64-bit key, ``site`` the stream
    id, ``step`` the training-step counter.  Build with ``dropout_spec``."""

    __slots__ = ()

    def __new__(cls, thr, scale, seed, site, step):
        return tuple.__new__(cls, (int(thr), float(scale), int(seed), int(site), int(step)))

    thr = property(lambda s: s[0])
    scale = property(lambda s: s[1])
    seed = property(lambda s: s[2])
    site = property(lambda s: s[3])
    step = property(lambda s: s[4])

    def kw(self):
        """The extension's keyword arguments."""
        return dict(thr=self[0], seed=self[2], site=self[3], step=self[4])


def dropout_thr(p: float) -> int:
    """round(p·65536) clamped to [0, 65535]."""
    return max(0, min(65535, int(round(float(p) * 65536.0))))


def dropout_spec(p: float, seed: int, site: int, step: int):
    """The ``drop`` argument of the ops for probability ``p``, or None when p
    quantises to no dropout (thr == 0: the ops then take their plain paths)."""
    import numpy as np
    thr = dropout_thr(p)
    if thr == 0:
        return None
    scale = float(np.float32(65536.0) / np.float32(65536 - thr))
    return Dropout(thr, scale, seed & 0xFFFFFFFFFFFFFFFF, site & _U32, step & _U32)


def _as_drop(drop):
    if drop is None:
        return None
    d = drop if isinstance(drop, Dropout) else Dropout(*drop)
    return d if d.thr else None


def ref_dropout(t: torch.Tensor, drop) -> torch.Tensor:
    """drop(t) with the host-built mask, in t's dtype (differentiable)."""
    keep = philox_keep_mask(t.shape, drop.thr, drop.seed, drop.site, drop.step).to(t.device)
    return torch.where(keep, t * drop.scale, torch.zeros((), dtype=t.dtype, device=t.device))


# attention-probability dropout: one Philox call per 4-query × 4-key patch

ATTN_SITE0 = 0x10000  # attention sites are ATTN_SITE0 + layer (0 and 1 + 2i / 2 + 2i are taken)


def _attn_patch_words(g, seed: int, site: int, step: int):
    """The four Philox output words of the attention patches ``g`` (uint64 array
    of 64-bit patch indices): counter (g_lo, g_hi, site, step), key = seed halves."""
    import numpy as np
    g = np.asarray(g, dtype=np.uint64)
    return philox4x32_10((g & np.uint64(_U32), g >> np.uint64(32), site, step), (seed & _U32, (seed >> 32) & _U32))


def philox_attn_keep_mask(B: int, H: int, S: int, thr8: int, seed: int, site: int, step: int,
                          bh0: int = 0) -> torch.Tensor:
    """The attention-dropout keep mask as the flash kernels draw it
    (csrc/hip/philox.h), built on the host: bool [B, H, S, S], True = kept,
    indexed [b, h, query, key] (entries above the causal diagonal are drawn
    too; attention never reads them).

    One Philox4x32-10 call serves a patch of 4 queries × 4 keys: counter =
    (g_lo, g_hi, site, step) with g = ((b·H + h)·P + q//4)·P + k//4 as a 64-bit
    value, P = S/4 (rounded up when S is no multiple of 4, which only the
    reference paths see); key = (low, high) half of ``seed``.  Element (q, k)
    takes output word q % 4, bits 8·(k % 4) … + 7, and is kept iff that byte ≥
    ``thr8`` = round(p·256): p is quantised to 1/256.  ``bh0`` is added to
    b·H + h (a slice of a larger batch; the tests reach g ≥ 2^32 with it)."""
    import numpy as np
    if not 0 <= thr8 <= 255 or min(B, H, S) < 1:
        raise ValueError(f"philox_attn_keep_mask: thr8 in [0, 255] and positive sizes required, got {(B, H, S, thr8)}")
    P = (S + 3) // 4
    u = np.uint64
    bh = (np.arange(B * H, dtype=np.uint64) + u(bh0)).reshape(-1, 1, 1)
    q4 = np.arange(P, dtype=np.uint64).reshape(1, -1, 1)
    k4 = np.arange(P, dtype=np.uint64).reshape(1, 1, -1)
    g = (bh * u(P) + q4) * u(P) + k4  # [BH, P, P]
    w = np.stack(_attn_patch_words(g, seed, site, step), axis=-1)  # [BH, P, P, 4 (q % 4)]
    byte = (w[..., None] >> (np.arange(4, dtype=np.uint64) * u(8))) & u(0xFF)  # [BH, P, P, q % 4, k % 4]
    keep = (byte >= u(thr8)).transpose(0, 1, 3, 2, 4).reshape(B * H, 4 * P, 4 * P)[:, :S, :S]
    return torch.from_numpy(np.ascontiguousarray(keep)).reshape(B, H, S, S)


def attn_dropout_thr(p: float) -> int:
    """round(p·256) clamped to [0, 255]."""
    return max(0, min(255, int(round(float(p) * 256.0))))


def attn_dropout_spec(p: float, seed: int, site: int, step: int):
    """The ``drop`` argument of ``attention`` / ``qkv_attention`` for probability
    ``p``: a ``Dropout`` whose ``thr`` is thr8 = round(p·256) (attention dropout
    is quantised to 1/256) and whose ``scale`` is fp32 256 / (256 − thr8); None
    when thr8 == 0.  ``site``: ``ATTN_SITE0`` + layer."""
    import numpy as np
    thr = attn_dropout_thr(p)
    if thr == 0:
        return None
    scale = float(np.float32(256.0) / np.float32(256 - thr))
    return Dropout(thr, scale, seed & 0xFFFFFFFFFFFFFFFF, site & _U32, step & _U32)


# ----------------------------------------------------------------------------
# linear with direct-to-arena weight gradient
# ----------------------------------------------------------------------------

class _LinearFn(torch.autograd.Function):
    """y = x W^T (+ b) on the hand-written gemm_nt (csrc/hip/gemm_nt4.hip, bias
    fused in the register epilogue) where its shape contract holds.

    Backward: dX on gemm_nt (as F.linear(dY, Wᵀ)), dW on gemm_dw4 written
    straight into the parameter's slice of the flat gradient arena (no
    separate gradient tensor, no AccumulateGrad add kernel), then the bucketed
    all-reduce is signalled that the parameter is ready.  The bias gradient is
    a HIP column reduction."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        ctx.b = b
        return _fwd_gemm(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        K = x.shape[-1]
        Fo = dy.shape[-1]
        dy2 = dy.reshape(-1, Fo)
        x2 = x.reshape(-1, K)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _input_grad(dy2, w).view(x.shape)
        dw = _weight_grad(w, dy2, x2) if ctx.needs_input_grad[1] else None
        db = None
        if ctx.has_b and ctx.needs_input_grad[2]:
            if use_hip(dy2):
                gd = _arena_grads((ctx.b,))
                db = _native.require_hip().bias_grad(dy2.contiguous(), out=gd[0] if gd else None)
                if gd is not None:
                    _signal_ready((ctx.b,))
                    db = None
            else:
                db = dy2.float().sum(0).to(dy.dtype)
        return dx, dw, db


_WS = {}


def _workspace(device, numel):
    """Grow-only bf16 scratch per device (split-K partials)."""
    buf = _WS.get(device)
    if buf is None or buf.numel() < numel:
        buf = torch.empty(numel, dtype=torch.bfloat16, device=device)
        _WS[device] = buf
    return buf[:numel]


def _splitk(tokens: int, m: int, n: int) -> int:
    """Token-slice count for dW = dY^T X: aim for ≥256 output tiles of 256² (one per CU).

    The LM-head dW (50304×1024 → 786 tiles, K = 65536) is past that target but
    still runs 6-8 % faster as 4 token slices (tools/dw_probe.py, tuned).
    Padding the vocabulary to 50432 so gemm_dw takes it measured 6.10 ms (4
    slices) vs 6.35 ms here (tools/lm_dw_probe.py): not worth untuned
    forward / dX shapes for 0.16 % of the step."""
    if tokens < 8192:
        return 1
    tiles = max(1, (m * n) // 65536)
    if 256 <= tiles < 2048:
        return 4 if tokens >= 32768 and tokens % 4 == 0 else 1
    s = 1
    while s < 8 and tiles * s < 256 and tokens % (2 * s) == 0 and tokens // (2 * s) >= 2048:
        s *= 2
    return s


_DX_TN = [True]

# Every forward-layout GEMM (y = x·Wᵀ (+ b): QKV / proj / fc2 forward, the
# input-gradient GEMMs as F.linear(dY, Wᵀ), the LM head) on the hand-written
# gemm_nt4 instead of hipBLASLt, where its shape contract holds (M, N % 256,
# K % 128, or N % 256 = 128 like the 50304-column LM head).  Default since the
# row-accumulator schedules (profiles/r3_gemm_nt4_rows.md): no hipBLASLt kernel
# in the step.  (Test hook: 0 keeps the library for the GEMMs without a fused
# epilogue, 1 routes all of them, any larger value routes those with K ≤ it.)
_NT_ALL = [1]


def _fwd_gemm(x, w, b=None):
    """F.linear(x, w, b) — on gemm_nt4 under _NT_ALL when the shapes allow."""
    if (_NT_ALL[0] and (_NT_ALL[0] == 1 or x.shape[-1] <= _NT_ALL[0])
            and x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
            and x.is_contiguous() and w.is_contiguous() and (b is None or b.dtype == torch.bfloat16)):
        x2 = x.reshape(-1, x.shape[-1])
        m = _native.require_hip()
        if m.gemm_nt_supported(x2.shape[0], w.shape[0], w.shape[1]):
            return m.gemm_nt(x2, w, b).view(*x.shape[:-1], w.shape[0])
    return F.linear(x, w, b)


def _input_grad(dy2, w):
    """dX = dY·W as the forward's GEMM form F.linear(dY, Wᵀ) on gemm_nt.

    gemm_nt reads both operands K-contiguous; the explicit Wᵀ copy is ≤ 8 M
    elements per projection and runs in the LDS-tiled HIP transpose
    (csrc/hip/transpose.hip) at the HBM rate."""
    if _DX_TN[0] and dy2.is_cuda:
        return _fwd_gemm(dy2, transpose(w))
    return dy2 @ w


def _live_wt(w):
    """The arena's prebuilt Wᵀ of ``w`` (parallel.flat.FlatParams.enable_wt) while
    it is live (inside the trainer's wt_scope), else None."""
    t = getattr(w, "_pdo_wt", None)
    if t is not None and t[0].wt_live:
        return t[1]
    return None


def _transposable(w) -> bool:
    return (w.is_cuda and w.dtype == torch.bfloat16 and w.dim() == 2 and w.shape[0] % 64 == 0
            and w.shape[1] % 64 == 0 and w.is_contiguous())


def transpose(w, out=None):
    """Contiguous Wᵀ of a 2-D tensor (HIP kernel for bf16 with 64-multiple dims).

    (Measured, round 3: the step's 97 transposes prefetched on a side stream
    under the forward GEMMs made the step 1 ms slower — 148.2 vs 147.2 ms,
    profiles/r3_attention_variants_a5.md — so they stay in-stream.)"""
    if out is None:
        wt = _live_wt(w)
        if wt is not None:
            return wt
    if _transposable(w):
        if out is not None:
            return _native.require_hip().transpose(w, out)
        return _native.require_hip().transpose(w)
    return w.t().contiguous()


def _weight_grad(w, dy2, x2):
    """dW = dy2ᵀ·x2.  Straight into the flat arena when the parameter allows it
    (returns None), else as a tensor for autograd to accumulate.

    (A/B on 1×MI355X: issuing these GEMMs on a side HIP stream to overlap the
    memory-bound backward kernels gained nothing — 394.5k vs 394.7k tok/s — and
    stalled one run on cross-stream allocator reuse; they stay in-stream.)"""
    Fo, K = dy2.shape[1], x2.shape[1]
    if not _direct_ok(w):
        # a gradient tensor for autograd to accumulate (the tied LM head / embedding
        # weight): HIP dW GEMM where its shape contract holds (incl. the 50304-row
        # vocabulary's half-height tile row: 5.42 vs 6.41 ms alone, tools/lm_dw_probe.py;
        # in the step 159.08 / 159.20 vs 159.24 / 159.44 ms, tools/gpu.sh soab)
        if (_HIP_DW[0] and dy2.is_cuda and dy2.dtype == torch.bfloat16 and dy2.is_contiguous()
                and x2.is_contiguous()):
            g = torch.empty(Fo, K, device=dy2.device, dtype=dy2.dtype)
            if _native.require_hip().gemm_dw(dy2, x2, g, False):
                return g
        s = _splitk(dy2.shape[0], Fo, K) if use_hip(dy2) else 1
        if s == 1:
            return dy2.t() @ x2
        T = dy2.shape[0] // s
        part = torch.bmm(dy2.view(s, T, Fo).transpose(1, 2), x2.view(s, T, K),
                         out=_workspace(dy2.device, s * Fo * K).view(s, Fo, K))
        g = torch.empty(Fo, K, device=dy2.device, dtype=dy2.dtype)
        _native.require_hip().splitk_add(part, g, False)
        return g
    if _dw_queue.push(w, dy2, x2):
        return None  # runs, and signals, in flush_weight_grads
    _weight_grad_now(w, dy2, x2)
    w._pdo_ready(w)
    return None


def _weight_grad_now(w, dy2, x2):
    """The arena dW of one parameter on its own launch (split-K gemm_dw, or the library)."""
    if not (_HIP_DW[0] and dy2.is_cuda and w.grad.dtype == torch.bfloat16 and dy2.is_contiguous()
            and x2.is_contiguous() and _native.require_hip().gemm_dw(dy2, x2, w.grad, True)):
        _weight_grad_lib(w, dy2, x2)


# dW on the HIP token-major GEMM (csrc/hip/gemm_dw.hip) where its shape
# contract holds (M, N % 256, tokens % 64); hipBLASLt otherwise.  Measured at
# the GPT-2-medium B=64 shapes (tools/dw_probe.py --pdo-only): qkv 375 vs 390 µs,
# proj 131 vs 160, fc1 462 vs 505, fc2 468 vs 506 (hipBLASLt tuned + HIP fold).
_HIP_DW = [True]


def _weight_grad_lib(w, dy2, x2):
    """Arena dW on hipBLASLt: batched token-slice GEMM + HIP fold, or addmm_."""
    Fo, K = dy2.shape[1], x2.shape[1]
    g = w.grad.view(Fo, K)
    s = _splitk(dy2.shape[0], Fo, K)
    if s > 1:
        # long-K / few-tile dW: batched GEMM over token slices + fused fold into the arena
        T = dy2.shape[0] // s
        part = torch.bmm(dy2.view(s, T, Fo).transpose(1, 2), x2.view(s, T, K),
                         out=_workspace(dy2.device, s * Fo * K).view(s, Fo, K))
        _native.require_hip().splitk_add(part, g, True)
    else:
        g.addmm_(dy2.t(), x2)


def _direct_ok(p) -> bool:
    g = p.grad
    return (getattr(p, "_pdo_direct", False) and g is not None and g.is_contiguous()
            and torch.is_grad_enabled() is False)


def _arena_grads(params):
    """The parameters' arena gradient slices when every one of them takes a
    direct write (bf16 flat arena, see parallel.flat), else None.  Kernels that
    reduce a parameter gradient (LayerNorm γ/β, biases) then accumulate straight
    into the arena — no gradient tensor, no AccumulateGrad add kernel."""
    out = []
    for p in params:
        if p is None or not _direct_ok(p) or p.grad.dtype != torch.bfloat16:
            return None
        out.append(p.grad.view(-1))
    return out


class deferred_reductions:
    """Scope (the trainer's backward) in which the bias / norm-weight gradient
    column sums that kernels reduce into the arena are queued and run in a few
    batched launches (``flush_deferred``: before each bucket all-reduce, and on
    exit) — csrc/hip/bind.cpp colsum_or_defer."""

    def __init__(self, device):
        self.on = torch.device(device).type == "cuda" and _native.ops_mode() != "torch"
        self.prev = False

    def __enter__(self):
        if self.on:
            self.prev = _native.require_hip().colsum_defer(True)
        return self

    def __exit__(self, *exc):
        if self.on:
            _native.require_hip().colsum_defer(self.prev)  # off: flushes the queue


def flush_deferred():
    """Run the queued weight gradients and column sums now (stream-ordered; a
    no-op when none)."""
    flush_weight_grads()
    m = _native.hip_ext()
    if m is not None and m.colsum_pending():
        m.colsum_flush()


# ----------------------------------------------------------------------------
# grouped weight gradients
# ----------------------------------------------------------------------------
# Inside ``deferred_weight_grads`` (the trainer's backward) the arena dW GEMMs are
# queued with their operands held alive and run as ONE launch per group
# (csrc/hip/gemm_dw4.hip gemm_dw4_grouped): a workgroup owns one 256 × 256 output
# tile over the whole token axis, so nothing is split, no partial is written and
# nothing is folded, and a group whose tiles fill whole rounds of one workgroup
# per CU keeps every CU busy.  A single GEMM has too few tiles for that (GPT-2-
# medium: 48 / 16 / 64 / 64) and has to invent parallelism with split-K.
#
# The operands are read at the flush, later than today.  Nothing in the backward
# writes to them in between: dy2 / x2 are saved activations or gradients that the
# producing kernel wrote before _weight_grad was called; the residual-stream dh
# that _LinearResFn / _NTMLPFn hand on as an alias is only read downstream
# (layernorm_bwd_add writes a fresh tensor), autograd's in-place accumulation
# needs a sole owner of the storage (the queue holds one more), and scale_dev_
# runs on the LM head's dh before any consumer sees it.
#
# (Test hooks: _DW_GROUPED off = every dW on its own launch, as outside the scope;
# _DW_CUS overrides the device's CU count; _DW_CAP_BYTES the held-operand cap.)
_DW_GROUPED = [True]
_DW_CUS = [0]
_DW_CAP_BYTES = [16 << 30]  # GPT-2-medium's 4-layer group holds ≈ 8.6 GB of operands
_DW_MIN_ROUNDS = 3          # a launch boundary drains the chip: whole groups of ≥ 3 rounds
_DW_FILL = 0.94             # gemm_dw's own threshold for "the last round is nearly full"


def dw_tiles(M: int, N: int) -> int:
    """Output tiles (256 × 256, a half-height last row allowed) of an [M, N] dW."""
    return ((M + 255) // 256) * (N // 256)


def dw_should_flush(tiles, held_bytes: int, cus: int, cap_bytes: int, min_rounds: int = _DW_MIN_ROUNDS) -> bool:
    """The flush rule after a push, a pure function of the queued tile counts:
    flush when the tiles make whole rounds of one workgroup per CU (a positive
    multiple of ``cus``, at least ``min_rounds`` of them), or when the held operand
    bytes pass the cap."""
    total = sum(tiles)
    if total > 0 and total % cus == 0 and total >= min_rounds * cus:
        return True
    return held_bytes > cap_bytes


def dw_grouped_prefix(tiles, cus: int, fill: float = _DW_FILL) -> int:
    """How many leading queue entries a flush runs grouped: the longest prefix
    whose last round of ``cus`` workgroups is at least ``fill`` full.  The rest (a
    remainder that would leave CUs idle for a whole round) take the per-GEMM
    split-K path, so no shape runs slower than on its own."""
    best, total = 0, 0
    for i, t in enumerate(tiles):
        total += t
        last = total % cus or cus
        if total > 0 and last >= fill * cus:
            best = i + 1
    return best


class _DWQueue:
    def __init__(self):
        self.depth = 0       # nested deferred_weight_grads scopes
        self.entries = []    # (w, dy2, x2): the tensors stay alive until the flush
        self.tiles = []
        self.held = 0
        self.cus = 0
        self.n_grouped = 0   # problems run grouped so far (tests, probes)

    def push(self, w, dy2, x2) -> bool:
        """Queue the arena dW of ``w`` when it is within the grouped kernel's
        contract; False = the caller runs it now."""
        if not (self.depth and _DW_GROUPED[0] and _HIP_DW[0] and dy2.is_cuda and dy2.dtype == torch.bfloat16
                and x2.dtype == torch.bfloat16 and w.grad.dtype == torch.bfloat16 and dy2.is_contiguous()
                and x2.is_contiguous() and dy2.dim() == 2 and x2.dim() == 2):
            return False
        T, M, N = dy2.shape[0], dy2.shape[1], x2.shape[1]
        if x2.shape[0] != T or w.grad.numel() != M * N:
            return False
        if not _native.require_hip().gemm_dw_grouped_ok(T, M, N):
            return False
        if not self.cus:
            self.cus = _DW_CUS[0] or torch.cuda.get_device_properties(dy2.device).multi_processor_count
        self.entries.append((w, dy2, x2))
        self.tiles.append(dw_tiles(M, N))
        self.held += (dy2.numel() + x2.numel()) * 2
        if dw_should_flush(self.tiles, self.held, self.cus, _DW_CAP_BYTES[0]):
            self.flush()
        return True

    def flush(self):
        if not self.entries:
            return
        entries, tiles, cus = self.entries, self.tiles, self.cus
        self.entries, self.tiles, self.held, self.cus = [], [], 0, 0  # a ready hook may flush again
        k = dw_grouped_prefix(tiles, cus)
        if k:
            m = _native.require_hip()
            outs = [w.grad.view(dy2.shape[1], x2.shape[1]) for w, dy2, x2 in entries[:k]]
            if not m.gemm_dw_grouped([e[1] for e in entries[:k]], [e[2] for e in entries[:k]], outs, [True] * k):
                raise RuntimeError("gemm_dw_grouped rejected a queued weight gradient")
            self.n_grouped += k
        for w, dy2, x2 in entries[k:]:
            _weight_grad_now(w, dy2, x2)
        for w, _, _ in entries:
            w._pdo_ready(w)


_dw_queue = _DWQueue()


class deferred_weight_grads:
    """Scope (the trainer's backward) in which the arena weight-gradient GEMMs
    are queued and run grouped (above).  They are flushed when the queued tiles
    fill whole rounds, when the held operands pass the cap, by
    ``flush_deferred`` (before a bucket all-reduce) and on exit; a parameter's
    ``_pdo_ready`` fires after the flush that ran it."""

    def __init__(self, device):
        self.on = torch.device(device).type == "cuda" and _native.ops_mode() != "torch"

    def __enter__(self):
        if self.on:
            _dw_queue.depth += 1
        return self

    def __exit__(self, *exc):
        if self.on:
            _dw_queue.depth -= 1
            if _dw_queue.depth == 0:
                if exc and exc[0] is not None:
                    _dw_queue.entries, _dw_queue.tiles, _dw_queue.held = [], [], 0  # a failed backward: drop, do not launch
                else:
                    _dw_queue.flush()


def flush_weight_grads():
    """Run the queued weight gradients now and signal their parameters ready."""
    _dw_queue.flush()


def _signal_ready(params):
    for p in params:
        p._pdo_ready(p)


def linear(x, w, b=None):
    if use_hip(x):
        return _LinearFn.apply(x, w, b)
    return F.linear(x, w, b)


