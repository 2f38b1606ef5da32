"""Bit-exact and per-element float64 checks of the ResNet autograd nodes and their routes
(paddle_operator_amd/ops/resnet.py): the layer that wires the convolution, GEMM, BatchNorm and pooling
kernels into a training step.  The kernels themselves are held to their contracts by
test_conv_exact_gpu.py, test_bn_kernels_gpu.py, test_bn_eval_gpu.py, test_gemm_nt_exact_gpu.py and
test_gemm_dw_exact_gpu.py; this file imports their builders and checkers and applies them one level up,
where a norm over a whole tensor cannot see a dropped pixel, a ReLU bitmask shifted by a byte, a residual
gradient masked twice or not at all, a compact stride-2 gradient added at (2b, 2a), an arena write that
overwrites, or a BatchNorm that takes the epilogue partials of another gradient tensor.
test_resnet_nodes_cpu.py validates the builders, references and expected-value functions below and shows
the checkers rejecting each of those mistakes.

Route table.  Every case asserts the autograd node classes reachable from grad_fn (nodes() / assert_route
of test_gpt2_nodes_gpu.py), the link counters _BN_LINK_USED, _RES_MASK_USED, _DS_COMPACT_USED (links()),
and, where the node classes do not show the kernel, the extension calls made (calls()).  Hooks are the
one-element lists of ops/resnet.py, set by hooks() inside try / finally.  Shapes, the smallest at which
each route exists: T256 = N 4, 8 x 8 (gemm_nt's M % 256); T147 = N 3, 7 x 7, ragged (gemm_nt and gemm_dw
decline); a stride-2 block on N 2, 16 x 32 -> 8 x 16 (non-square: an H / W swap shows); a stride-2 block
on N 3, 14 x 14 -> 7 x 7 (the compact GEMM declines).

    op            route                                              selected by                              forced by
    conv forward  implicit GEMM, tile stats                          3x3, stride 2, or Kout <= 128             shape
                  gemm_nt_stats (EPI 9), 8-wave and 4-wave           1x1 s1, Kout > 128, T % 256 = 0;          shape
                                                                     Cin 64 / Cin >= 256
                  gemm_nt then the BN stats pass                                                              _GEMM_BN_STATS = False
                  framework conv                                     conv_ok fails (C 32), NCHW input          _HIP_CONV = False
    conv dX       gemm_nt / gemm_nt_add / gemm_nt_add(mask=)         1x1 s1, Cin > 128, T % 256 = 0            shape, fork, _RES_MASK
                  conv_dgrad(add), mask applied by _apply_bitmask    else                                      T147, Cin 64
                  conv_dgrad_bn then _BNLink                         input is a linked BN output               _BN_LINK
                  compact gemm_nt then _CompactGradLink then         1x1 s2 of a forked input, To % 256 = 0    _DS_COMPACT; declined
                  conv_stride2_add                                                                             at 14 x 14
                  dy is None (only the alias has a gradient),        y unused                                  graph
                  with and without mask and compact part
    conv dW       gemm_dw                                            1x1 s1, ceil(K/256) (C/256) >= 8,         shape
                                                                     T % 64 = 0 (C 2048, K 512, T256)
                  conv_wgrad after gemm_dw declines                  same channels, T147                       shape
                  conv_wgrad returned / conv_wgrad(out=p.grad)       _direct_cl_ok                             FlatParams live or not
    conv weights  shadow plus _pdo_shadow_t / cast plus per-         shadow_scope live                         scope
                  backward transpose
    BN            _BNActFn stats pass / from tile stats              producer gave st                          bn_act vs conv_bn_act
                  backward from bn_act_bwd_part (link) / stats pass  link taken                                _BN_LINK
                  residual with _ResMaskLink (dres = dy unmasked)    fork plus residual                        _RES_MASK
                  / masked dres
                  bitmask mode through mlink (downsample BN)         as_residual                               _DS_FUSED = False
                  framework fallback                                 C % 8 != 0, eval with grad                _BN_FUSED = False
    block tail    _BNActBNResFn / two-pass with mlink / two-pass plain                                        _DS_FUSED, _RES_MASK
    stem          _StemFn then _BNReluPoolFn                                                                   default, N 2 16 x 24 image
                  _StemFn then _BNActFn then _MaxPool3s2Fn                                                     _STEM_POOL = False
                  framework conv then bn_act then pool               x.requires_grad, odd H                    _HIP_STEM = False
    pool          _GAPFn / framework                                 C % 8                                     shape

Eval-mode routes belong to test_bn_eval_gpu.py.

(a) Bit-exact on integer grids: gradient transport through the links.  Operands are those of
test_conv_exact_gpu.py (activations in [-3, 3], weights in [-1, 1], gradients in [-2, 2], joining gradients
and accumulate bases in [-8, 8]; the compact-downsample case uses [-15, 15] so that its sums need their
roundings), exact_bound asserted per case.  Expected values are float64 F.conv2d / autograd on the CPU
pushed through the contracts read from the epilogues:

  y                    RNE(conv).
  dX, gemm_nt_add      contraction length = Kout.  On the 4-wave mainloop (Kout % 128 = 0, Kout >= 256) the
                       addend joins the fp32 product: RNE(P + dalias (.) keep).  On the 8-wave ring (Kout 64,
                       128) it joins the staged bf16 product: RNE(RNE(P) + dalias (.) keep)  (gemm_nt.hip's
                       header; both pinned by test_gemm_nt_exact_gpu.py).  The mask only zeroes addend
                       elements, which is exact on either mainloop: masked in the epilogue (EPI 6) or before
                       it (EPI 4 on dy (.) keep) gives the same bits, on random data too.
  dX, conv_dgrad(add)  RNE(P + dalias (.) keep); the mask is applied to the addend first (_apply_bitmask).
  dX past a BN link    conv_dgrad_bn, then dx + dalias in the framework: RNE(RNE(P) + dalias).
  dX, compact          stride2_add_ref(RNE(P1), RNE(Pds)): two roundings at the pixels (2a, 2b), one
                       elsewhere.  With _DS_COMPACT off, or where the compact GEMM declines (14 x 14), the
                       downsample's zero-filled RNE(Pds) is conv1's addend: RNE(P1 + RNE(Pds)) on the 4-wave
                       mainloop and on conv_dgrad(add).  The compact case runs conv1 with Kout 256 so that the
                       two contracts differ (CPU file: in at least 5 % of the stride-2 pixels); on the 8-wave
                       ring the zero-filled form has the compact form's bits.
  dW                   the exact fp32 sum; gemm_dw: RNE_bf16 of it (one split at T256, asserted).  Into the
                       arena: base + dW with a non-zero integer base, every other arena element untouched.

A BatchNorm with gamma = 0 and integer beta is exact: y = act(beta [+ residual]), dx = 0, dres = dy (.) mask,
dbeta = sum g; dgamma is held to check_bwd's band.  The mask (beta + residual > 0) is known without a kernel.

(b) Per-element float64 bands on random data, node by node inside models.resnet.Bottleneck and the stem.
tap() records every node's saved tensors and, through Node.register_hook, its gradient inputs and outputs;
capture() records the extension calls whose results autograd does not keep (the tile statistics, the
backward partials, the compact gradient).  Each node is compared with the float64 of that node alone from
its observed bf16 inputs:

  BatchNorm forward    stats pass: check_fwd with fwd_stats_bound.  From tile statistics: the observed
                       partials are the node's input, so the reference mean and variance are tiles_stats' of
                       those partials with its bounds (check_fwd's body with the statistics given:
                       check_fwd_given), and the partials themselves are held to the float64 partials of x
                       with test_conv_exact_gpu.py's tolerance for them.  check_running for the running
                       statistics, the saved bitmask against y > 0.
  BatchNorm backward   check_bwd with the saved mean and invstd.  g = dy (.) (the forward's own y > 0).  With
                       the link the sums come from conv_dgrad_bn's tile partials: a tile adds at most 16 rows
                       per thread, 2 butterflies and 4 wave totals (conv_epilogue: LT = 22), then
                       bn_act_bwd_part's chain_rows over the partial rows.
  fused tail           the checks of test_bn_pair on both sides.
  stem                 check_stem on the observed stem output (its own partials), and the node's saved
                       statistics, pooled output and dx by the same formulas from the observed partials.
  convolutions         |got - ref| <= K 2^-24 sum |terms| plus the output type's half spacing (out_bound); a
                       route that rounds twice (above) adds the half spacing of the inner product.
  link contracts       under _ResMaskLink the BatchNorm's residual gradient is its dy bit for bit (the same
                       tensor) and the mask appears only in conv1's dX; under mlink the downsample BatchNorm's
                       g is dy (.) keep with bn3's mask; under _CompactGradLink the downsample _ConvFn returns
                       no input gradient.

(c) Identity and failure behaviour of the hand-offs: a linked BN output with two consumers, a forked input
with a third consumer, shadow weights, the arena route, a second backward through a retained graph (every
link is consumed by the first: it must have the bits of a backward with the links switched off), a
no_grad forward.

Not held here: the framework convolution's rounding (C 32, NCHW input, _HIP_CONV off, the framework stem):
only its route and finite results; at C 32 its bf16 output lay 1.97 bounds from float64, so the project
states no contract for it.  Every route of the table is reachable at the shapes above.

Measured on an MI355X (each test prints its figures; 74 tests, 9 s, the slowest 2.4 s: the first framework
convolution).  Every bit-exact and bit-identity check holds and no check exposed a defect in an op or a
kernel.  Worst error as a share of the counted bound inside the blocks: tile partials 3e-4 of their
tolerance; mean 0 - 0.12, invstd 0.08 - 0.20, running statistics 0.05 - 0.42; dgamma 0.007 - 0.055, dbeta at
most 0.009 (exact on integer gradients); y and dx of every BatchNorm and convolution 0.76 - 0.996, which is
the output's own bf16 rounding (half a spacing is up to 2^-8 of the value); dW 0.001 - 0.02.  Grid shares
(CPU file): the compact and the zero-filled downsample gradient differ in 21.8 % of the stride-2 pixels,
RNE_bf16(dW) of the gemm_dw cases from the exact dW in most elements.
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import test_bn_kernels_gpu as bk
import test_conv_exact_gpu as cx
from test_bn_kernels_gpu import (EPS, L_MAX, MOM, U, Report, bn_bwd_ref, chain_rows, chain_stats, check_bwd, check_fwd,
                                 check_running, check_stem, fwd_stats_bound, near_zero, out_bound, rows_of, same_bits,
                                 tiles_stats, unpack_mask, zero_near)
from test_conv_exact_gpu import (ADD_MAX, DY_MAX, KRSC, LIM, NHWC, W_MAX, X_MAX, check_bits, conv_ref, exact_bound,
                                 exact_f32, grads_ref, ints, nhwc, rne_bf16, stride2_add_ref)
from test_gpt2_nodes_gpu import assert_route, calls, nodes, route_ok

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
LT = 22        # conv_epilogue's tile_sum: 16 rows per thread, 2 butterflies, at most 4 wave totals
BIG = 15       # operand magnitude of the compact-downsample grid case
TRACK = ("conv_fwd", "gemm_nt", "gemm_nt_stats", "gemm_nt_add", "conv_dgrad", "conv_dgrad_bn", "conv_wgrad", "gemm_dw",
         "conv_stride2_add", "conv_weight_t", "transpose", "bn_act_fwd", "bn_act_fwd_tiles", "bn_act_bwd", "bn_act_bwd_part")


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _ops():
    from paddle_operator_amd import ops
    return ops


def _R():
    from paddle_operator_amd.ops import resnet
    return resnet


def record(line):
    print(f"[resnet-nodes] {line}")


# ---------------------------------------------------------------------------------------------
# routes, hooks, counters
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def hooks(**kw):
    """Set the one-element test hooks of ops.resnet for the block; restored after it."""
    R = _R()
    cells = {k: getattr(R, k) for k in kw}
    saved = {k: c[0] for k, c in cells.items()}
    try:
        for k, v in kw.items():
            cells[k][0] = v
        yield
    finally:
        for k, c in cells.items():
            c[0] = saved[k]


class links:
    """The link counters (_BN_LINK_USED, _RES_MASK_USED, _DS_COMPACT_USED) moved inside the block."""

    def __enter__(self):
        self.start = self._now()
        return self

    def __exit__(self, *exc):
        return False

    @staticmethod
    def _now():
        R = _R()
        return (R._BN_LINK_USED[0], R._RES_MASK_USED[0], R._DS_COMPACT_USED[0])

    @property
    def used(self):
        return tuple(b - a for a, b in zip(self.start, self._now()))


def nonzero(count):
    return {k: v for k, v in count.items() if v}


@contextlib.contextmanager
def capture(m, *names):
    """Record (args, result) of the extension's functions `names` as the ops call them: the tile statistics,
    the backward partials and the compact gradient are inputs of a node that autograd does not keep."""
    log = {n: [] for n in names}
    real = {n: getattr(m, n) for n in names}

    def wrap(n):
        def f(*a, **kw):
            out = real[n](*a, **kw)
            log[n].append((a, kw, out))
            return out
        return f

    try:
        for n in names:
            setattr(m, n, wrap(n))
        yield log
    finally:
        for n in names:
            setattr(m, n, real[n])


WATCH = ("_ConvFnBackward", "_BNActFnBackward", "_BNActBNResFnBackward", "_StemFnBackward", "_BNReluPoolFnBackward",
         "_MaxPool3s2FnBackward", "_GAPFnBackward")


def graph_nodes(*tensors):
    """Every autograd node reachable from the tensors' grad_fn, in a fixed depth-first order."""
    seen, order, stack = set(), [], [t.grad_fn for t in reversed(tensors)]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        order.append(fn)
        stack.extend(f for f, _ in reversed(fn.next_functions))
    return order


def tap(*tensors):
    """One record per project node reachable from the tensors: class, the node, its saved tensors, and after
    the backward its gradient inputs `gi` (what the node returned) and outputs `go` (what it received)."""
    recs = []
    for fn in graph_nodes(*tensors):
        name = type(fn).__name__
        if name not in WATCH:
            continue
        r = dict(cls=name[:-len("Backward")], fn=fn, saved=fn.saved_tensors, runs=0)

        def hook(gi, go, r=r):
            r["gi"], r["go"] = gi, go
            r["runs"] += 1
        fn.register_hook(hook)
        recs.append(r)
    return recs


def of_class(recs, cls):
    return [r for r in recs if r["cls"] == cls]


def producer_of(fn, k=0):
    return fn.next_functions[k][0]


# ---------------------------------------------------------------------------------------------
# builders and expected values (CPU, float64; validated by test_resnet_nodes_cpu.py)
# ---------------------------------------------------------------------------------------------
def nt4(k):
    """The GEMM of contraction length k runs the 4-wave mainloop (gemm_nt.hip nt4_path): its addend epilogues
    round once; the 8-wave ring rounds the product first."""
    return k % 128 == 0 and k >= 256


def keep_of(shape, seed):
    """A reproducible keep mask [N, C, H, W] (bool), about half set, no structure along any axis."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) < 0.5


def pack_mask(keep):
    """keep [N, C, H, W] bool -> the ReLU bitmask bytes of the channels_last tensor: bit j of byte i is
    element 8 i + j in (n, h, w, c) order (unpack_mask's inverse)."""
    flat = keep.permute(0, 2, 3, 1).reshape(-1, 8).to(torch.int32)
    return (flat << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


def rne2(p, add):
    """Two roundings: the product to bf16, then the sum."""
    return rne_bf16(rne_bf16(p).double() + add)


def dx_expect(p, add, route, kout):
    """conv dX on the grid.  p = the exact product, add = the (already masked) joining gradient or None,
    route = "gemm" (gemm_nt / gemm_nt_add, contraction kout), "dgrad" (conv_dgrad(add)) or "dgrad_bn"
    (conv_dgrad_bn, then dx + dalias)."""
    if add is None:
        return rne_bf16(p)
    if route == "dgrad" or (route == "gemm" and nt4(kout)):
        return rne_bf16(p + add)
    assert route in ("gemm", "dgrad_bn")
    return rne2(p, add)


def zero_fill(c, H, W):
    """A compact [N, C, Ho, Wo] gradient at the pixels (2a, 2b) of a zero [N, C, H, W]."""
    out = torch.zeros(c.shape[0], c.shape[1], H, W, dtype=c.dtype)
    out[:, :, ::2, ::2] = c
    return out


def ds_expect(p1, pds, compact, route="gemm", kout=256):
    """The forked input's gradient of a stride-2 downsample pair on the grid: p1 = conv1's exact product
    [N, C, H, W], pds = the downsample's exact compact product [N, C, Ho, Wo]."""
    if compact:
        return stride2_add_ref(rne_bf16(p1).double(), rne_bf16(pds).double())
    return dx_expect(p1, zero_fill(rne_bf16(pds).double(), p1.shape[2], p1.shape[3]), route, kout)


def relu_res_expect(beta, res):
    """gamma = 0: y = relu(beta + residual) exactly, and its keep mask."""
    pre = beta.view(1, -1, 1, 1) + res
    return rne_bf16(pre.clamp_min(0.0)), pre > 0


@functools.lru_cache(maxsize=None)
def ds_case(N, C, H, W, K1, Kd, amax=BIG):
    """The compact-downsample grid case: x [N, C, H, W], conv1 1x1 s1 C -> K1, downsample 1x1 s2 C -> Kd,
    integers in [-amax, amax]; float64 products of both input gradients and both weight gradients."""
    seed = 7 * N + 11 * C + 13 * H + 17 * W + K1 + Kd
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, w1, wd = ints((N, C, H, W), amax, seed), ints((K1, C, 1, 1), amax, seed + 1), ints((Kd, C, 1, 1), amax, seed + 2)
    dy1, dyd = ints((N, K1, H, W), amax, seed + 3), ints((N, Kd, Ho, Wo), amax, seed + 4)
    assert exact_bound(C, amax, amax) < LIM                                             # forwards
    assert exact_bound(K1, amax, amax) + exact_bound(Kd, amax, amax) + 256 < LIM        # dX and their sum
    assert exact_bound(N * H * W, amax, amax) < LIM                                     # dW
    p1, dw1 = grads_ref(x, w1, dy1, 1)
    pfull, dwd = grads_ref(x, wd, dyd, 2)
    pds = pfull[:, :, ::2, ::2].contiguous()
    assert bool((zero_fill(pds, H, W) == pfull).all())
    return dict(x=x, w1=w1, wd=wd, dy1=dy1, dyd=dyd, y1=conv_ref(x, w1, 1), yd=conv_ref(x, wd, 2), p1=p1, pds=pds,
                dw1=dw1, dwd=dwd)


def dev_keep(keep):
    return pack_mask(keep).cuda()


def conv_param(w):
    return torch.nn.Parameter(cx.dev_f32(w))


class ConvArena:
    """A convolution weight between two other parameters in an fp32 FlatParams arena.  The whole gradient
    arena holds a non-integer sentinel, the weight's slice an integer base: after a backward the slice must
    be base + dW and every other element must keep its bits."""

    def __init__(self, w, base):
        from paddle_operator_amd.parallel.flat import FlatParams
        self.mod = torch.nn.Module()
        self.mod.pre = torch.nn.Parameter(torch.zeros(24, device="cuda"))
        self.mod.w = conv_param(w)
        self.mod.post = torch.nn.Parameter(torch.zeros(40, device="cuda"))
        self.flat = FlatParams(self.mod, dtype=torch.float32, device="cuda")
        n = self.flat.grads.numel()
        self.sentinel = (torch.arange(n, dtype=torch.float32, device="cuda") % 97) + 0.25
        self.flat.grads.copy_(self.sentinel)
        self.slot = next(s for s in self.flat.slots if s.name == "w")
        self.mod.w.grad.copy_(base.to(torch.float32).cuda())
        self.ready = 0
        self.mod.w._pdo_ready = self._count

    def _count(self, p):
        self.ready += 1

    def expect(self, value):
        e = self.sentinel.clone()
        self.flat._view(e, self.slot).copy_(value.to(torch.float32).cuda())
        return e

    def check(self, value, what):
        torch.cuda.synchronize()
        check_bits(nhwc(self.mod.w.grad), nhwc(value.to(torch.float32)), KRSC, f"{what}: arena slice")
        check_bits(self.flat.grads, self.expect(value), ("arena element",), f"{what}: whole arena")


# ---------------------------------------------------------------------------------------------
# (a) 1. _ConvFn alone: every dX and dW route
# ---------------------------------------------------------------------------------------------
T256_512 = (4, 256, 8, 8, 512, 1, 1)
# name: (shape, alias, arena, dX route, extension calls of one forward and one backward)
#   alias: "none" | "add" (a joining gradient) | "mask" (a joining gradient under a keep mask)
CONV_NODE = {
    "t256-k512": (T256_512, "none", False, "gemm", dict(gemm_nt_stats=1, gemm_nt=1, transpose=1, conv_wgrad=1)),
    "t256-k512-add-arena": (T256_512, "add", True, "gemm", dict(gemm_nt_stats=1, gemm_nt_add=1, transpose=1, conv_wgrad=1)),
    "t256-k512-mask": (T256_512, "mask", False, "gemm", dict(gemm_nt_stats=1, gemm_nt_add=1, transpose=1, conv_wgrad=1)),
    # Kout 64: the forward stays on the implicit GEMM, dX is the 8-wave ring's (two roundings with an addend)
    "t256-k64-add": ((4, 256, 8, 8, 64, 1, 1), "add", False, "gemm", dict(conv_fwd=1, gemm_nt_add=1, transpose=1, conv_wgrad=1)),
    "t256-k64-mask-arena": ((4, 256, 8, 8, 64, 1, 1), "mask", True, "gemm",
                            dict(conv_fwd=1, gemm_nt_add=1, transpose=1, conv_wgrad=1)),
    # Cin 64: the 8-wave gemm_nt_stats forward; dX on conv_dgrad, the mask applied by _apply_bitmask
    "t256-c64-mask": ((4, 64, 8, 8, 256, 1, 1), "mask", False, "dgrad",
                      dict(gemm_nt_stats=1, conv_dgrad=1, conv_weight_t=1, conv_wgrad=1)),
    "t147-k512-add": ((3, 256, 7, 7, 512, 1, 1), "add", False, "dgrad", dict(conv_fwd=1, conv_dgrad=1, conv_weight_t=1, conv_wgrad=1)),
    "t147-3x3-mask-arena": ((3, 64, 7, 7, 64, 3, 1), "mask", True, "dgrad",
                            dict(conv_fwd=1, conv_dgrad=1, conv_weight_t=1, conv_wgrad=1)),
    "s2-3x3-arena": ((2, 128, 8, 12, 128, 3, 2), "none", True, "dgrad", dict(conv_fwd=1, conv_dgrad=1, conv_weight_t=1, conv_wgrad=1)),
    "t256-c2048-gemm_dw": ((4, 2048, 8, 8, 512, 1, 1), "none", False, "gemm", dict(gemm_nt_stats=1, gemm_nt=1, transpose=1, gemm_dw=1)),
    "t256-c2048-gemm_dw-arena": ((4, 2048, 8, 8, 512, 1, 1), "add", True, "gemm",
                                 dict(gemm_nt_stats=1, gemm_nt_add=1, transpose=1, gemm_dw=1)),
    # gemm_dw is asked and declines 147 tokens: conv_wgrad, straight into the arena
    "t147-c2048-declined-arena": ((3, 2048, 7, 7, 512, 1, 1), "none", True, "dgrad",
                                  dict(conv_fwd=1, conv_dgrad=1, conv_weight_t=1, gemm_dw=1, conv_wgrad=1)),
}


@functools.lru_cache(maxsize=None)
def big_case(shape, amax=BIG):
    """test_conv_exact_gpu.case() with activations and output gradients in [-amax, amax]: the gemm_dw cases,
    whose exact dW (up to 256 amax^2) then needs its bf16 rounding."""
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, M = cx.geometry(shape)
    seed = sum(v * 29 ** i for i, v in enumerate(shape)) % (1 << 31)
    x, w = ints((N, C, H, W), amax, seed), ints((K, C, R, R), W_MAX, seed + 1)
    dy, add = ints((N, K, Ho, Wo), amax, seed + 2), ints((N, C, H, W), ADD_MAX, seed + 3)
    base = ints((K, C, R, R), ADD_MAX, seed + 4)
    assert 256 * exact_bound(R * R * C, amax, W_MAX) < LIM                # forward and its tile sums
    assert exact_bound(R * R * K, amax, W_MAX, ADD_MAX) < LIM             # input gradient (+ add)
    assert exact_bound(M, amax, amax, ADD_MAX) < LIM                      # weight gradient (+ out)
    dx, dw = grads_ref(x, w, dy, st)
    return dict(x=x, w=w, dy=dy, add=add, base=base, y=conv_ref(x, w, st), dx=dx, dw=dw)


def conv_node_expect(name):
    """Expected bits of one CONV_NODE case: y, dX, and dW (as the value added to the gradient)."""
    shape, alias, arena, route, want = CONV_NODE[name]
    N, C, H, W, K, R, st = shape
    c = big_case(shape) if "gemm_dw" in want and "conv_wgrad" not in want else cx.case(shape)
    keep = keep_of((N, C, H, W), 5 + K) if alias == "mask" else None
    add = None if alias == "none" else (c["add"] * keep if keep is not None else c["add"])
    dw = rne_bf16(c["dw"]).double() if "gemm_dw" in want and "conv_wgrad" not in want else c["dw"]
    return dict(c=c, keep=keep, y=rne_bf16(c["y"]), dx=dx_expect(c["dx"], add, route, K), dw=dw)


@pytest.mark.parametrize("name", list(CONV_NODE))
def test_conv_node_routes_exact(cuda, name):
    """_ConvFn on each forward, dX and dW route: y, the tile statistics, dX and dW to the bit; the route by
    the extension calls made; a masked joining gradient through a hand-made _ResMaskLink."""
    R, m = _R(), _m()
    shape, alias, arena, route, want = CONV_NODE[name]
    N, C, H, W, K, Rr, st = shape
    pad, Ho, Wo, M = cx.geometry(shape)
    e = conv_node_expect(name)
    c = e["c"]
    T = N * H * W
    assert ("gemm_nt_stats" in want) == (Rr == 1 and st == 1 and R._gemm_fwd_1x1(m, T, C, K))
    assert (route == "gemm") == (Rr == 1 and st == 1 and R._gemm_dgrad_1x1(m, T, C, K))
    assert ("gemm_dw" in want) == (Rr == 1 and st == 1 and R._gemm_wgrad_1x1(C, K))
    if "gemm_dw" in want:
        assert m.gemm_dw_splits(T, K, C) == (1 if T % 64 == 0 else 0)
    ar = ConvArena(c["w"], c["base"]) if arena else None
    w = ar.mod.w if arena else conv_param(c["w"])
    x = cx.dev_bf16(c["x"]).requires_grad_()
    fork = alias != "none"
    rl = R._ResMaskLink() if alias == "mask" else None
    with links() as lk, calls(m, *TRACK) as n:
        y, stt, xa = R._ConvFn.apply(x, w, st, pad, True, fork, rl, None, None)
        assert_route(y, ["_ConvFn"])
        outs, grads = [y], [cx.dev_bf16(c["dy"])]
        if fork:
            dalias = cx.dev_bf16(c["add"])
            outs.append(xa)
            grads.append(dalias)
            if rl is not None:
                rl.give(dalias, dev_keep(e["keep"]))
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
    assert nonzero(n) == want, f"{name}: extension calls {nonzero(n)}"
    assert lk.used == (0, 1 if alias == "mask" else 0, 0)
    what = f"_ConvFn {name}"
    check_bits(nhwc(y.detach()), nhwc(e["y"]), NHWC, f"{what}: y")
    tile = m.gemm_nt_stats_rows(C) if "gemm_nt_stats" in want else m.conv_tile_rows(K)
    assert tile <= 256 and stt is not None and not stt.requires_grad
    cx.check_tile_stats(stt, y.detach(), K, tile, what)
    check_bits(nhwc(x.grad), nhwc(e["dx"]), NHWC, f"{what}: dX")
    if arena:
        ar.check(c["base"] + e["dw"], f"{what}: dW")
        assert ar.ready == (1 if "conv_wgrad" in want else 0)     # gemm_dw's dW is returned and added by autograd
    else:
        assert w.grad.dtype == torch.float32
        check_bits(nhwc(w.grad), nhwc(exact_f32(e["dw"])), KRSC, f"{what}: dW")


# ---------------------------------------------------------------------------------------------
# (a) 2. identity-block wiring
# ---------------------------------------------------------------------------------------------
IDENT = {"gemm-T256": (4, 256, 8, 8, 64), "bitmask-T147": (3, 64, 7, 7, 64)}     # N, Cin, H, W, Kout of conv1


@functools.lru_cache(maxsize=None)
def ident_case(key):
    N, C, H, W, K = IDENT[key]
    c = cx.case((N, C, H, W, K, 1, 1))
    seed = 97 + C + H
    beta = ints((C,), 3, seed)
    z, w3 = ints((N, 64, H, W), X_MAX, seed + 1), ints((C, 64, 1, 1), W_MAX, seed + 2)
    dyo = ints((N, C, H, W), ADD_MAX, seed + 3)
    yo, keep = relu_res_expect(beta, c["x"])
    assert 0.2 < float(keep.double().mean()) < 0.8
    return dict(c=c, beta=beta, z=z, w3=w3, dyo=dyo, yo=yo, keep=keep, g=dyo * keep)


def bn_module(C, gamma=None, beta=None):
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        if gamma is not None:
            bn.weight.copy_(gamma.to(torch.float32))
        if beta is not None:
            bn.bias.copy_(beta.to(torch.float32))
    return bn


def conv_module(w, stride=1):
    K, C, R, _ = w.shape
    conv = torch.nn.Conv2d(C, K, R, stride=stride, padding=(R - 1) // 2, bias=False).cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_(w.to(torch.float32))
    return conv


def run_identity(key, res_mask, random=False):
    """x -> _ConvFn(fork): y to a weighted loss, xa the residual of conv_bn_act(conv3, bn3, z, residual=xa).
    Returns everything observable (CPU)."""
    R, ops, m = _R(), _ops(), _m()
    N, C, H, W, K = IDENT[key]
    k = ident_case(key)
    c = k["c"]
    if random:
        g = torch.Generator().manual_seed(3 + C)
        rnd = lambda *s: torch.randn(*s, generator=g).to(BF16).double()
        xv, w1, dy1, dyo, z, w3 = (rnd(N, C, H, W), rnd(K, C, 1, 1) / 8, rnd(N, K, H, W), rnd(N, C, H, W), rnd(N, 64, H, W),
                                   rnd(C, 64, 1, 1) / 8)
        bn3 = bn_module(C, 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g))
    else:
        xv, w1, dy1, dyo, z, w3 = c["x"], c["w"], c["dy"], k["dyo"], k["z"], k["w3"]
        bn3 = bn_module(C, torch.zeros(C), k["beta"])
    conv3 = conv_module(w3)
    w1p = conv_param(w1)
    x = cx.dev_bf16(xv).requires_grad_()
    with hooks(_RES_MASK=res_mask), links() as lk, calls(m, *TRACK) as n:
        rl = R._ResMaskLink() if R._RES_MASK[0] else None
        y1, _, xa = R._ConvFn.apply(x, w1p, 1, 0, True, True, rl, None, None)
        if rl is not None:
            xa._pdo_rlink = rl
        out = ops.conv_bn_act(conv3, bn3, cx.dev_bf16(z), relu=True, residual=xa)
        assert_route((y1, out), ["_ConvFn", "_BNActFn"])
        recs = tap(y1, out)
        bn = of_class(recs, "_BNActFn")[0]
        torch.autograd.backward([y1, out], [cx.dev_bf16(dy1), cx.dev_bf16(dyo)])
        torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.detach().cpu()
    return dict(used=lk.used, calls=nonzero(n), y1=cpu(y1), out=cpu(out), dx=cpu(x.grad), dw1=cpu(w1p.grad),
                bn_saved=[cpu(t) for t in bn["saved"]], bn_gi=[cpu(t) for t in bn["gi"]], bn_go=cpu(bn["go"][0]),
                dres_is_dy=bn["gi"][3].data_ptr() == bn["go"][0].data_ptr(), dgamma=cpu(bn3.weight.grad),
                dbeta=cpu(bn3.bias.grad), dw3=cpu(conv3.weight.grad))


@pytest.mark.parametrize("key", list(IDENT))
def test_identity_wiring_exact(cuda, key):
    """conv1's dX = RNE(dy W (+) dy_out (.) keep) with the mask applied in the GEMM epilogue (Cin 256) or by
    _apply_bitmask before conv_dgrad (Cin 64, T147), with _RES_MASK on and off: both the expectation's bits.
    Under the link the BatchNorm's residual gradient is its dy itself; without it, dy (.) keep."""
    N, C, H, W, K = IDENT[key]
    k = ident_case(key)
    c = k["c"]
    gemm = key.startswith("gemm")
    assert gemm == bool(_R()._gemm_dgrad_1x1(_m(), N * H * W, C, K))
    want_dx = dx_expect(c["dx"], k["g"], "gemm" if gemm else "dgrad", K)
    res = {}
    for on in (True, False):
        r = res[on] = run_identity(key, on)
        what = f"identity {key} _RES_MASK={on}"
        assert r["used"] == (0, 1 if on else 0, 0), what
        assert ("gemm_nt_add" in r["calls"]) == gemm and ("conv_dgrad" in r["calls"]) == (not gemm)
        check_bits(nhwc(r["y1"]), nhwc(rne_bf16(c["y"])), NHWC, f"{what}: y")
        check_bits(nhwc(r["out"]), nhwc(k["yo"]), NHWC, f"{what}: relu(beta + x)")
        x3, mask, mean, invstd, gam, _ = r["bn_saved"]
        M = N * H * W
        assert torch.equal(unpack_mask(mask, M, C), rows_of(k["keep"])), f"{what}: the saved bitmask is not beta + x > 0"
        check_bits(nhwc(r["dx"]), nhwc(want_dx), NHWC, f"{what}: conv1 dX")
        check_bits(nhwc(r["dw1"]), nhwc(exact_f32(c["dw"])), KRSC, f"{what}: conv1 dW")
        dres = r["bn_gi"][3]
        if on:
            assert r["dres_is_dy"], f"{what}: the residual gradient is not the BatchNorm's dy tensor"
            check_bits(nhwc(dres), nhwc(k["dyo"].to(BF16)), NHWC, f"{what}: dres = dy unmasked")
        else:
            assert bool((dres.double() == k["g"]).all()), f"{what}: dres is not dy (.) keep"
        rep = Report(what)
        Lb = chain_stats(M, C, True)
        assert Lb <= L_MAX and float(k["g"].abs().sum((0, 2, 3)).max()) < LIM
        out = (r["bn_gi"][0], None, r["dgamma"], r["dbeta"])
        check_bwd(rep, "bn3 ", out, rows_of(k["g"]), rows_of(x3).double(), mean, invstd, gam.double(), Lb, False)
        rep.exact("bn3 dx = 0", bool((r["bn_gi"][0] == 0).all()))
        rep.exact("bn3 dbeta exact", torch.equal(r["dbeta"].double(), k["g"].sum((0, 2, 3))))
        rep.check()
    for n in ("dx", "dw1", "dgamma", "dbeta", "dw3", "out"):
        assert same_bits(res[True][n], res[False][n]), f"identity {key}: {n} differs between _RES_MASK on and off"


@pytest.mark.parametrize("key", list(IDENT))
def test_res_mask_on_off_bit_identical_on_random_data(cuda, key):
    """Applying a 0 / 1 mask to the addend is exact and the mainloop is the same: on random data the
    epilogue-masked route and the BatchNorm-masked route give the same bits everywhere."""
    a, b = run_identity(key, True, random=True), run_identity(key, False, random=True)
    assert a["used"] == (0, 1, 0) and b["used"] == (0, 0, 0)
    for n in ("y1", "out", "dx", "dw1", "dgamma", "dbeta", "dw3"):
        assert same_bits(a[n], b[n]), f"identity {key}, random data: {n} differs between _RES_MASK on and off"
    assert same_bits(a["bn_gi"][0], b["bn_gi"][0])
    assert float(a["dx"].float().abs().mean()) > 0.1


# ---------------------------------------------------------------------------------------------
# (a) 3. the compact downsample hand-off
# ---------------------------------------------------------------------------------------------
# name: (N, C, H, W, K1, Kd), _DS_COMPACT, the contract, dX route of conv1
DS_CASES = {
    "compact-16x32": ((2, 256, 16, 32, 256, 512), True, "compact", "gemm"),
    "zero-filled-16x32": ((2, 256, 16, 32, 256, 512), False, "one", "gemm"),
    "declined-14x14": ((3, 256, 14, 14, 256, 512), True, "one", "dgrad"),
}


def run_ds_pair(k, compact_hook, dalias=None, keep=None, use_y=True):
    """x -> _ConvFn(conv1, fork, slink); xa -> the 1x1 stride-2 _ConvFn(clink = that link).  Optional: a
    further gradient of xa (dalias, with a keep mask through a hand-made _ResMaskLink), y unused."""
    R, m = _R(), _m()
    w1, wd = conv_param(k["w1"]), conv_param(k["wd"])
    x = cx.dev_bf16(k["x"]).requires_grad_()
    with hooks(_DS_COMPACT=compact_hook), links() as lk, calls(m, *TRACK) as n:
        sl = R._CompactGradLink() if R._DS_COMPACT[0] else None
        rl = R._ResMaskLink() if keep is not None else None
        y1, _, xa = R._ConvFn.apply(x, w1, 1, 0, True, True, rl, sl, None)
        yd, _, _ = R._ConvFn.apply(xa, wd, 2, 0, True, False, None, None, sl)
        outs, grads = [yd], [cx.dev_bf16(k["dyd"])]
        if use_y:
            outs.append(y1)
            grads.append(cx.dev_bf16(k["dy1"]))
        if dalias is not None:
            da = cx.dev_bf16(dalias)
            outs.append(xa)
            grads.append(da)
            if rl is not None:
                rl.give(da, dev_keep(keep))
        recs = tap(*outs)
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
    ds = next(r for r in of_class(recs, "_ConvFn") if r["saved"][1].shape[0] == k["wd"].shape[0])
    return dict(used=lk.used, calls=nonzero(n), y1=y1.detach(), yd=yd.detach(), dx=x.grad, dw1=w1.grad, dwd=wd.grad,
                ds_dx=ds["gi"][0])


@pytest.mark.parametrize("name", list(DS_CASES))
def test_compact_downsample_exact(cuda, name):
    """The forked input's gradient of a stride-2 downsample pair: compact = RNE(P1) then RNE(. + RNE(Pds)) at
    the pixels (2a, 2b) of a non-square image; zero-filled = RNE(P1 + RNE(Pds)).  The compact downsample
    _ConvFn returns no input gradient."""
    dims, hook, contract, route = DS_CASES[name]
    N, C, H, W, K1, Kd = dims
    m, R = _m(), _R()
    k = ds_case(*dims)
    To = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
    assert (contract == "compact") == (hook and bool(m.gemm_nt_supported(To, C, Kd)))
    assert (route == "gemm") == bool(R._gemm_dgrad_1x1(m, N * H * W, C, K1)) and nt4(K1)
    r = run_ds_pair(k, hook)
    what = f"downsample pair {name}"
    assert r["used"] == (0, 0, 1 if contract == "compact" else 0), what
    assert ("conv_stride2_add" in r["calls"]) == (contract == "compact")
    assert (r["ds_dx"] is None) == (contract == "compact"), f"{what}: the downsample's own input gradient"
    check_bits(nhwc(r["y1"]), nhwc(rne_bf16(k["y1"])), NHWC, f"{what}: y1")
    check_bits(nhwc(r["yd"]), nhwc(rne_bf16(k["yd"])), NHWC, f"{what}: yd")
    check_bits(nhwc(r["dx"]), nhwc(ds_expect(k["p1"], k["pds"], contract == "compact", route, K1)), NHWC, f"{what}: dX")
    check_bits(nhwc(r["dw1"]), nhwc(exact_f32(k["dw1"])), KRSC, f"{what}: conv1 dW")
    check_bits(nhwc(r["dwd"]), nhwc(exact_f32(k["dwd"])), KRSC, f"{what}: downsample dW")


# ---------------------------------------------------------------------------------------------
# (a) 4. dy is None: only the alias carries a gradient
# ---------------------------------------------------------------------------------------------
UNUSED_Y = [("alias", False), ("alias", True), ("alias+compact", False), ("alias+compact", True), ("compact", False)]


@pytest.mark.parametrize("part,mask", UNUSED_Y, ids=[f"{p}-{'mask' if k else 'plain'}" for p, k in UNUSED_Y])
def test_conv_node_unused_output_exact(cuda, part, mask):
    """y unused: the forked input's gradient is the alias gradient (.) keep [+ the compact downsample part at
    the pixels (2a, 2b)], exact; no weight gradient.  (A mask needs an alias gradient to apply to.)"""
    dims = (2, 256, 16, 32, 256, 512)
    N, C, H, W, K1, Kd = dims
    k = ds_case(*dims)
    R, m = _R(), _m()
    dal = ints((N, C, H, W), BIG, 401)
    keep = keep_of((N, C, H, W), 402) if mask else None
    masked = dal * keep if mask else dal
    what = f"unused y, {part}, mask={mask}"
    if part == "alias":
        w1 = conv_param(k["w1"])
        x = cx.dev_bf16(k["x"]).requires_grad_()
        rl = R._ResMaskLink() if mask else None
        with links() as lk, calls(m, *TRACK) as n:
            _, _, xa = R._ConvFn.apply(x, w1, 1, 0, True, True, rl, None, None)
            da = cx.dev_bf16(dal)
            if rl is not None:
                rl.give(da, dev_keep(keep))
            xa.backward(da)
        assert nonzero(n) == dict(gemm_nt_stats=1) and lk.used == (0, int(mask), 0) and w1.grad is None
        check_bits(nhwc(x.grad), nhwc(masked.to(BF16)), NHWC, what)
        return
    r = run_ds_pair(k, True, dalias=None if part == "compact" else dal, keep=keep, use_y=False)
    assert r["used"] == (0, int(mask), 1) and r["dw1"] is None and r["ds_dx"] is None
    assert r["calls"].get("conv_stride2_add") == 1 and "gemm_nt_add" not in r["calls"] and "conv_dgrad" not in r["calls"]
    base = torch.zeros_like(dal) if part == "compact" else masked
    check_bits(nhwc(r["dx"]), nhwc(stride2_add_ref(base, rne_bf16(k["pds"]).double())), NHWC, what)
    check_bits(nhwc(r["dwd"]), nhwc(exact_f32(k["dwd"])), KRSC, f"{what}: downsample dW")


# ---------------------------------------------------------------------------------------------
# (a) 5. / (c) a linked BatchNorm output that is forked, or consumed twice
# ---------------------------------------------------------------------------------------------
def check_bn_node_bwd(rep, tag, rec, ypos, L, dy=None, sums=None, want_dres=False, gamma_beta=None):
    """check_bwd on a tapped _BNActFn node: g = (its observed dy) (.) ypos, the saved x, mean and invstd."""
    x, _, mean, invstd, w, _ = (None if t is None else t.detach() for t in rec["saved"])
    dy = rec["go"][0] if dy is None else dy
    g = rows_of(dy).double() * ypos
    dw, db = (rec["gi"][1], rec["gi"][2]) if gamma_beta is None else gamma_beta
    out = (rec["gi"][0], rec["gi"][3] if want_dres else None, dw, db)
    x64 = rows_of(x).double()
    if sums is None:
        sums = bk.bwd_sums(g, x64 - mean.double(), L, exact_s1=False)
    check_bwd(rep, tag, out, g, x64, mean, invstd, w.detach().double(), L, want_dres, sums=sums)
    return g


@pytest.mark.parametrize("data", ("grid", "random"))
def test_fork_of_linked_bn_output(cuda, data):
    """A BatchNorm output that a forking implicit-GEMM convolution consumes: conv_dgrad_bn, then dx + dalias in
    the framework, RNE(RNE(P) + dalias) on the grid.  The parked partials belong to another tensor: the link
    is not taken and the BatchNorm's gradients stay inside the stats-pass band for the gradient it received."""
    R, ops, m = _R(), _ops(), _m()
    N, C, H, W, K = 3, 64, 7, 7, 64
    M = N * H * W
    g = torch.Generator().manual_seed(11)
    if data == "grid":
        choices = torch.tensor([-2.0, -1.0, 1.0, 2.0, 3.0], dtype=F64)      # never 0: the mask is beta > 0 exactly
        beta = choices[torch.randint(0, 5, (C,), generator=g)]
        bn = bn_module(C, torch.zeros(C), beta)
        x0 = torch.randn(N, C, H, W, generator=g).to(BF16).double()
        w, dy, dal = ints((K, C, 3, 3), W_MAX, 12), ints((N, K, H, W), DY_MAX, 13), ints((N, C, H, W), ADD_MAX, 14)
        assert exact_bound(9 * K, DY_MAX, W_MAX, ADD_MAX) < LIM
    else:
        bn = bn_module(C, 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g))
        x0, dy, dal = (torch.randn(s, generator=g).to(BF16).double() for s in ((N, C, H, W), (N, K, H, W), (N, C, H, W)))
        w = (torch.randn(K, C, 3, 3, generator=g) / 24).to(BF16).double()
    wp = conv_param(w)
    xin = cx.dev_bf16(x0).requires_grad_()
    with links() as lk, calls(m, *TRACK) as n:
        yb = ops.bn_act(bn, xin, relu=True)
        assert getattr(yb, "_pdo_bn", None) is not None
        y, _, xa = R._ConvFn.apply(yb, wp, 1, 1, True, True, None, None, None)
        assert_route((y, xa), ["_ConvFn", "_BNActFn"])
        recs = tap(y, xa)
        torch.autograd.backward([y, xa], [cx.dev_bf16(dy), cx.dev_bf16(dal)])
        torch.cuda.synchronize()
    assert lk.used == (0, 0, 0), "the link was taken although the gradient is dx + dalias"
    assert n["conv_dgrad_bn"] == 1 and n["bn_act_bwd"] == 1 and n["bn_act_bwd_part"] == 0 and n["bn_act_fwd"] == 1
    bnr, cv = of_class(recs, "_BNActFn")[0], of_class(recs, "_ConvFn")[0]
    what = f"fork of a linked BN output ({data})"
    ypos = rows_of(yb.detach()) > 0
    if data == "grid":
        xb = beta.clamp_min(0.0).view(1, C, 1, 1).expand(N, C, H, W).contiguous()
        check_bits(nhwc(yb.detach()), nhwc(xb.to(BF16)), NHWC, f"{what}: relu(beta)")
        p, dw = grads_ref(xb, w, dy, 1)
        check_bits(nhwc(cv["gi"][0]), nhwc(dx_expect(p, dal, "dgrad_bn", K)), NHWC, f"{what}: dX")
        check_bits(nhwc(wp.grad), nhwc(exact_f32(dw)), KRSC, f"{what}: dW")
        assert torch.equal(ypos.cpu(), rows_of((beta > 0).view(1, C, 1, 1).expand(N, C, H, W)))
    assert same_bits(bnr["go"][0], cv["gi"][0])
    L = chain_stats(M, C, True)
    assert L <= L_MAX
    rep = Report(what)
    check_bn_node_bwd(rep, "bn ", bnr, ypos, L, gamma_beta=(bn.weight.grad, bn.bias.grad))
    rep.exact("bn dx is x.grad", same_bits(bnr["gi"][0], xin.grad))
    rep.check()


def test_linked_bn_output_with_two_consumers(cuda):
    """Two implicit-GEMM convolutions consume one linked BatchNorm output and both park partials on its link:
    the BatchNorm receives dx1 + dx2, must not use either consumer's partials (_BN_LINK_USED unchanged), and
    its gradients stay inside the stats-pass band against g = (dx1 + dx2) (.) mask."""
    R, ops, m = _R(), _ops(), _m()
    N, C, H, W = 3, 64, 7, 7
    M = N * H * W
    g = torch.Generator().manual_seed(21)
    bn = bn_module(C, 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g))
    x0 = torch.randn(N, C, H, W, generator=g).to(BF16).double()
    ws = [(torch.randn(K, C, 3, 3, generator=g) / 24).to(BF16).double() for K in (64, 128)]
    dys = [torch.randn(N, K, H, W, generator=g).to(BF16).double() for K in (64, 128)]
    xin = cx.dev_bf16(x0).requires_grad_()
    with links() as lk, calls(m, *TRACK) as n:
        yb = ops.bn_act(bn, xin, relu=True)
        ys = [R._ConvFn.apply(yb, conv_param(w), 1, 1, True)[0] for w in ws]
        recs = tap(*ys)
        torch.autograd.backward(ys, [cx.dev_bf16(d) for d in dys])
        torch.cuda.synchronize()
    assert lk.used == (0, 0, 0), "the BatchNorm took one consumer's partials for the sum of two gradients"
    assert n["conv_dgrad_bn"] == 2 and n["bn_act_bwd"] == 1 and n["bn_act_bwd_part"] == 0
    bnr, cvs = of_class(recs, "_BNActFn")[0], of_class(recs, "_ConvFn")
    assert len(cvs) == 2 and bnr["runs"] == 1
    total = cvs[0]["gi"][0].float() + cvs[1]["gi"][0].float()
    assert same_bits(bnr["go"][0], total.to(BF16)), "the BatchNorm's dy is not RNE(dx1 + dx2)"
    rep = Report("linked BN output, two consumers")
    L = chain_stats(M, C, True)
    check_bn_node_bwd(rep, "bn ", bnr, rows_of(yb.detach()) > 0, L, gamma_beta=(bn.weight.grad, bn.bias.grad))
    # the mistake this guards against is far outside the band: dx1 alone as g
    alone = bn_bwd_ref(rows_of(cvs[0]["gi"][0]).double() * (rows_of(yb.detach()) > 0), rows_of(bnr["saved"][0].detach()).double(),
                       bnr["saved"][2].double(), bnr["saved"][3].double(), bnr["saved"][4].detach().double())[0]
    assert float((rows_of(bnr["gi"][0]).double() - alone).abs().max()) > 0.05
    rep.check()


def test_forked_input_with_a_third_consumer_raises(cuda):
    """The forked input feeds the residual BatchNorm and something else: the gradient that reaches conv1 is a
    sum, not the BatchNorm's dy, and _ResMaskLink.take raises instead of masking it."""
    ops = _ops()
    N, C, H, W = 4, 256, 8, 8
    g = torch.Generator().manual_seed(31)
    conv1 = conv_module((torch.randn(64, C, 1, 1, generator=g) / 16).double())
    conv3 = conv_module((torch.randn(C, 64, 1, 1, generator=g) / 8).double())
    bn1, bn3 = bn_module(64), bn_module(C)
    x = cx.dev_bf16(torch.randn(N, C, H, W, generator=g).double()).requires_grad_()
    with links() as lk:
        out, xa = ops.conv_bn_act(conv1, bn1, x, fork=True)
        assert getattr(xa, "_pdo_rlink", None) is not None
        y = ops.conv_bn_act(conv3, bn3, out, relu=True, residual=xa)
        loss = y.float().sum() + (xa.float() * 0.5).sum()
        with pytest.raises(RuntimeError, match="residual mask hand-off"):
            loss.backward()
    assert lk.used[1] == 0 and x.grad is None


# ---------------------------------------------------------------------------------------------
# (a) 6. dbeta (and dgamma) into the arena with a base
# ---------------------------------------------------------------------------------------------
def bn_arena(mod, seed):
    """mod's parameters in an fp32 FlatParams arena whose gradients hold integers in [-8, 8] (the base)."""
    from paddle_operator_amd.parallel.flat import FlatParams
    flat = FlatParams(mod, dtype=torch.float32, device="cuda")
    base = ints((flat.grads.numel(),), ADD_MAX, seed).to(torch.float32).cuda()
    flat.grads.copy_(base)
    ready = {}
    for n, p in mod.named_parameters():
        ready[n] = 0

        def count(p, n=n):
            ready[n] += 1
        p._pdo_ready = count
    return flat, ready


def check_bn_arena(rep, tag, bn, base_w, base_b, g, x, mean, invstd, L):
    """bn.weight.grad / bn.bias.grad (arena slices that held base_w / base_b) after one backward with g."""
    x64, mu, inv = x.double(), mean.double(), invstd.double()
    xc = x64 - mu
    s1, s2, e_s1, e_s2 = bk.bwd_sums(g, xc, L)
    _, dg_ref, db_ref = bn_bwd_ref(g, x64, mu, inv, bn.weight.detach().double())
    _, e_dg, _ = bk.bwd_bound(s1, s2, e_s1, e_s2, g, xc, inv, bn.weight.detach().double(), x.shape[0])
    rep.add(tag + "dgamma into", bn.weight.grad, base_w.double() + dg_ref, e_dg + U * (base_w.double() + dg_ref).abs())
    rep.exact(tag + "dbeta = base + sum g", torch.equal(bn.bias.grad.double(), base_b.double() + db_ref))


@pytest.mark.parametrize("node", ("_BNActFn", "_BNActBNResFn", "_BNReluPoolFn"))
def test_bn_parameter_gradients_into_arena_with_base(cuda, node):
    """dbeta is an exact integer sum for an integer dy whatever the activations are: with a non-zero integer
    base in the fp32 arena the slice must hold base + sum g (an overwrite, a doubled add or another channel
    shows), dgamma base + its banded value; every parameter's ready fires once."""
    ops = _ops()
    g = torch.Generator().manual_seed(41)
    mod = torch.nn.Module()
    if node == "_BNActFn":
        N, C, H, W = 3, 64, 7, 7
        mod.bn = bn_module(C, 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g))
        xin = cx.dev_bf16(torch.randn(N, C, H, W, generator=g).double())
        run = lambda: ops.bn_act(mod.bn, xin, relu=True)
        bns = ["bn"]
    elif node == "_BNActBNResFn":
        N, C, H, W, K = 3, 64, 7, 7, 256
        mod.conv, mod.dconv = (conv_module((torch.randn(K, C, 1, 1, generator=g) / 8).double()) for _ in range(2))
        mod.bn, mod.dbn = (bn_module(K, 0.5 + torch.rand(K, generator=g), 0.2 * torch.randn(K, generator=g)) for _ in range(2))
        xin = cx.dev_bf16(torch.randn(N, C, H, W, generator=g).double())
        xa = cx.dev_bf16(torch.randn(N, C, H, W, generator=g).double())
        run = lambda: ops.conv_bn_ds_act(mod.conv, mod.bn, xin, mod.dconv, mod.dbn, xa)
        bns = ["bn", "dbn"]
    else:
        N, H, W = 2, 16, 24
        mod.conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().to(memory_format=torch.channels_last)
        mod.bn = bn_module(64, 0.5 + torch.rand(64, generator=g), 0.2 * torch.randn(64, generator=g))
        xin = cx.dev_bf16(torch.randn(N, 3, H, W, generator=g).double())
        run = lambda: ops.conv_bn_relu_maxpool(mod.conv, mod.bn, xin)
        bns = ["bn"]
    flat, ready = bn_arena(mod, 43)
    base = {n: p.grad.detach().clone() for n, p in mod.named_parameters()}
    with torch.autocast("cuda", dtype=BF16):
        y = run()
    assert_route(y, [node])
    rec = of_class(tap(y), node)[0]
    dyd = cx.dev_bf16(ints(tuple(y.shape), 4, 44))
    if node == "_BNActFn":
        # this backward recomputes the ReLU mask from x: dy is cleared where the float64 pre-activation lies
        # within the fp32 bound of zero, so the expected sum does not depend on which side the kernel puts it
        sv = [None if t is None else t.detach() for t in rec["saved"]]
        nz = near_zero(rows_of(sv[0]).double(), sv[2].double(), sv[3].double(), sv[4].double(), sv[5].double())
        dyd = bk.nhwc(zero_near(rows_of(dyd), nz).contiguous(), N, H, W)
    y.backward(dyd)
    torch.cuda.synchronize()
    gy = rows_of(dyd).double() * (rows_of(y.detach()) > 0)
    assert float(gy.abs().sum(0).max()) < LIM
    rep = Report(f"arena base, {node}")
    if node == "_BNActFn":
        x, _, mean, invstd, _, _ = rec["saved"]
        check_bn_arena(rep, "", mod.bn, base["bn.weight"], base["bn.bias"], gy, rows_of(x), mean, invstd, chain_stats(x.shape[0] * 49, 64, True))
    elif node == "_BNActBNResFn":
        x, r, _, mean, invstd, _, _, rmean, rinvstd, _, _ = rec["saved"]
        L = chain_stats(gy.shape[0], gy.shape[1], True)
        check_bn_arena(rep, "bn3 ", mod.bn, base["bn.weight"], base["bn.bias"], gy, rows_of(x), mean, invstd, L)
        check_bn_arena(rep, "ds ", mod.dbn, base["dbn.weight"], base["dbn.bias"], gy, rows_of(r), rmean, rinvstd, L)
    else:
        x, yp, xsel, arg, mean, invstd, _, _ = rec["saved"]
        L = chain_stats(gy.shape[0], 64, True)
        # the statistics run over the pooled tensors: g and the BatchNorm input at each window's maximum
        check_bn_arena(rep, "", mod.bn, base["bn.weight"], base["bn.bias"], gy, rows_of(xsel), mean, invstd, L)
    for n in bns:
        assert ready[n + ".weight"] == 1 and ready[n + ".bias"] == 1, (node, ready)
    rep.check()


# ---------------------------------------------------------------------------------------------
# the route table: node classes and counters of every row not asserted by a case above or below
# ---------------------------------------------------------------------------------------------
def rand_bf16(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def dev_cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def conv_bound(x, w, stride, kred):
    """(ref, e) of conv(x, w) in float64 on the CPU with e = kred 2^-24 sum |terms|."""
    x, w = x.detach().double().cpu(), w.detach().double().cpu()
    pad = (w.shape[-1] - 1) // 2
    ref = F.conv2d(x, w, stride=stride, padding=pad)
    return ref, kred * U * F.conv2d(x.abs(), w.abs(), stride=stride, padding=pad)


FWD_ROUTES = {
    # name: (N, C, H, W, K, NCHW input, hooks, node classes that ran / did not, extension calls)
    "implicit-k64": (4, 256, 8, 8, 64, False, {}, ["_ConvFn", "_BNActFn"], [], dict(conv_fwd=1, bn_act_fwd_tiles=1)),
    "stats-8wave": (4, 64, 8, 8, 256, False, {}, ["_ConvFn", "_BNActFn"], [], dict(gemm_nt_stats=1, bn_act_fwd_tiles=1)),
    "stats-4wave": (4, 256, 8, 8, 512, False, {}, ["_ConvFn", "_BNActFn"], [], dict(gemm_nt_stats=1, bn_act_fwd_tiles=1)),
    "gemm-then-stats-pass": (4, 256, 8, 8, 512, False, dict(_GEMM_BN_STATS=False), ["_ConvFn", "_BNActFn"], [],
                             dict(gemm_nt=1, bn_act_fwd=1)),
    "t147-implicit": (3, 256, 7, 7, 512, False, {}, ["_ConvFn", "_BNActFn"], [], dict(conv_fwd=1, bn_act_fwd_tiles=1)),
    "framework-c32": (4, 32, 8, 8, 64, False, {}, ["_BNActFn"], ["_ConvFn"], dict(bn_act_fwd=1)),
    # (the framework convolution of an NCHW input with a channels_last weight writes channels_last: the
    # BatchNorm stays on the HIP path)
    "framework-nchw": (4, 64, 8, 8, 64, True, {}, ["_BNActFn"], ["_ConvFn"], dict(bn_act_fwd=1)),
    "framework-hook": (4, 64, 8, 8, 64, False, dict(_HIP_CONV=False), ["_BNActFn"], ["_ConvFn"], dict(bn_act_fwd=1)),
    # without the fused BatchNorm nothing consumes tile statistics: conv_bn_act runs the framework pair
    "bn-framework-hook": (4, 64, 8, 8, 64, False, dict(_BN_FUSED=False), [], ["_ConvFn", "_BNActFn"], {}),
}


@pytest.mark.parametrize("name", list(FWD_ROUTES))
def test_conv_bn_forward_routes(cuda, name):
    """conv_bn_act's forward routes by node classes and extension calls; y of the convolution inside
    K 2^-24 sum |terms| of float64 (read back as the BatchNorm node's saved input where there is one), and a
    backward that leaves finite gradients and no link counter moved."""
    ops, m = _ops(), _m()
    N, C, H, W, K, nchw, hk, ran, not_ran, want = FWD_ROUTES[name]
    conv = conv_module(rand_bf16((K, C, 1, 1), 51, C ** -0.5).double())
    bn = bn_module(K)
    xv = rand_bf16((N, C, H, W), 52)
    x = (xv.cuda() if nchw else dev_cl(xv)).requires_grad_()
    with hooks(**hk), links() as lk, calls(m, *TRACK) as n, torch.autocast("cuda", dtype=BF16):
        y = ops.conv_bn_act(conv, bn, x)
        fwd = nonzero(n)
        names = assert_route(y, ran, not_ran)
        if "_ConvFn" in not_ran:
            assert any("Convolution" in s for s in names), sorted(names)
        if "_BNActFn" in not_ran:
            assert any("BatchNorm" in s for s in names), sorted(names)
        recs = tap(y)
        y.backward(dev_cl(rand_bf16(tuple(y.shape), 53)) if not nchw else rand_bf16(tuple(y.shape), 53).cuda())
        torch.cuda.synchronize()
    assert fwd == want, f"{name}: forward extension calls {fwd}"
    assert lk.used == (0, 0, 0)
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(conv.weight.grad).all())
    bnr = of_class(recs, "_BNActFn")
    if bnr and "_ConvFn" in ran:      # (the framework convolution's rounding is not the project's to state)
        ref, e = conv_bound(xv, conv.weight.to(BF16), 1, C)
        rep = Report(f"forward route {name}")
        rep.add("conv y", bnr[0]["saved"][0].detach().cpu(), ref, out_bound(ref, e))
        rep.check()


def test_bn_fallback_routes(cuda):
    """C % 8 != 0 and eval mode with autograd recording take the framework's BatchNorm, not _BNActFn."""
    ops = _ops()
    x12 = dev_cl(rand_bf16((2, 12, 5, 5), 61)).requires_grad_()
    with torch.autocast("cuda", dtype=BF16):
        y = ops.bn_act(bn_module(12), x12)
    assert_route(y, [], ["_BNActFn"])
    bn = bn_module(64).eval()
    x = dev_cl(rand_bf16((2, 64, 5, 5), 62)).requires_grad_()
    with torch.autocast("cuda", dtype=BF16):
        y = ops.bn_act(bn, x)
    assert_route(y, [], ["_BNActFn"])
    y.float().sum().backward()
    assert bool(torch.isfinite(x.grad).all())


def test_pool_routes(cuda):
    """_GAPFn and _MaxPool3s2Fn for C % 8 = 0, the framework's pools otherwise."""
    ops = _ops()
    x = dev_cl(rand_bf16((4, 64, 5, 5), 63)).requires_grad_()
    assert_route(ops.global_avg_pool(x), ["_GAPFn"])
    assert_route(ops.max_pool_3x3s2(x), ["_MaxPool3s2Fn"])
    x12 = dev_cl(rand_bf16((4, 12, 5, 5), 64)).requires_grad_()
    assert_route(ops.global_avg_pool(x12), [], ["_GAPFn"])
    assert_route(ops.max_pool_3x3s2(x12), [], ["_MaxPool3s2Fn"])
    # _GAPFn at 4 x 4: the mean of 16 integers and dy / 16 at every pixel are exact
    xv, dyv = ints((3, 64, 4, 4), 7, 65), ints((3, 64), 64, 66)
    x = cx.dev_bf16(xv).requires_grad_()
    y = ops.global_avg_pool(x)
    assert_route(y, ["_GAPFn"])
    check_bits(y.detach(), (xv.sum((2, 3)) / 16).to(BF16), ("n", "channel"), "_GAPFn y")
    y.backward(dyv.to(BF16).cuda())
    assert x.grad.is_contiguous(memory_format=torch.channels_last)
    check_bits(nhwc(x.grad), nhwc((dyv / 16).view(3, 64, 1, 1).expand(3, 64, 4, 4).to(BF16)), NHWC, "_GAPFn dx")


@pytest.mark.parametrize("why", ("requires_grad", "odd-H"))
def test_stem_route_selected_by_the_input(cuda, why):
    """An image that needs a gradient, or with an odd height, is outside _stem_ok: the framework convolution,
    then bn_act and the HIP pool."""
    ops, m = _ops(), _m()
    H = 15 if why == "odd-H" else 16
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().to(memory_format=torch.channels_last)
    bn = bn_module(64)
    x = dev_cl(rand_bf16((2, 3, H, 24), 67))
    if why == "requires_grad":
        assert m.stem_ok(2, H, 24, 3, 64)
        x.requires_grad_()
    else:
        assert not m.stem_ok(2, H, 24, 3, 64)
    assert not ops._stem_ok(conv, x)
    with links() as lk, calls(m, "stem_fwd", "bn_act_fwd", "maxpool3s2_fwd") as n, torch.autocast("cuda", dtype=BF16):
        y = ops.conv_bn_relu_maxpool(conv, bn, x)
        names = assert_route(y, ["_BNActFn", "_MaxPool3s2Fn"], ["_StemFn", "_BNReluPoolFn"])
        assert any("Convolution" in s for s in names)
        y.float().sum().backward()
    assert nonzero(n) == dict(bn_act_fwd=1, maxpool3s2_fwd=1) and lk.used == (0, 0, 0)
    assert bool(torch.isfinite(conv.weight.grad).all()) and (x.grad is not None) == (why == "requires_grad")


# ---------------------------------------------------------------------------------------------
# (b) node-by-node float64 bands inside real blocks
# ---------------------------------------------------------------------------------------------
CAPTURE = ("conv_fwd", "gemm_nt_stats", "stem_fwd", "bn_act_fwd", "bn_act_fwd_tiles", "bn_act_fwd_tiles_bnres",
           "bn_relu_pool_fwd_tiles", "bn_act_bwd", "bn_act_bwd_part", "conv_dgrad_bn", "conv_stride2_add", "gemm_dw")


def check_partials(rep, tag, st, x64, t):
    """Observed tile statistics [G, 2, C] against the float64 partials of x [M, C], with the tolerance
    test_conv_exact_gpu.py holds them to on non-integer data (rtol = atol = 2e-3)."""
    ref = bk.tile_partials(x64, t, F64)
    assert st.shape == ref.shape, f"{tag}: partials {tuple(st.shape)} for {tuple(ref.shape)}"
    ratio = (st.double() - ref).abs() / (cx.STATS_ATOL + cx.STATS_RTOL * ref.abs())
    rep.rows.append((tag + "partials", float(ratio.max())))


def check_fwd_given(rep, tag, x, w, b, eps, relu, y, mean, invstd, mean_t, var_t, e_mean, e_var, add=None, e_add=None):
    """check_fwd's body with the statistics given: the float64 mean and variance of the partials the node
    received (tiles_stats), not of x.  Returns the reference dict and e_v."""
    inv = (var_t + eps) ** -0.5
    pre = (x - mean_t) * inv * w + b
    if add is not None:
        pre = pre + add
    ref = dict(mean=mean_t, var=var_t, invstd=inv, pre=pre, y=pre.clamp_min(0.0) if relu else pre, e_mean=e_mean, e_var=e_var)
    e_inv = bk.invstd_bound(var_t, eps, e_var)
    e_v = bk.preact_bound(x, mean_t, inv, w, b, e_mean, e_inv)
    if add is not None:
        e_v = e_v + e_add + U * pre.abs()
    rep.add(tag + "mean", mean, mean_t, e_mean)
    rep.add(tag + "invstd", invstd, inv, e_inv)
    rep.add(tag + "y", y, ref["y"], out_bound(ref["y"], e_v))
    return ref, e_v


def audit_bn_forward(rep, tag, call, tiles, init):
    """One observed bn_act_fwd / bn_act_fwd_tiles call: mean, invstd, y, the running statistics and the
    bitmask against float64 of its own inputs.  Returns y > 0 as rows."""
    a, _, out = call
    if tiles:
        x, st, t, res, w, b, rm, rv, eps, mom, relu = a
    else:
        (x, res, w, b, rm, rv, eps, mom, relu), st = a, None
    y, mean, invstd, mask = out
    C = x.shape[1]
    x64, w64, b64, eps = rows_of(x).double(), w.detach().double(), b.detach().double(), bk.f32(eps)
    M = x64.shape[0]
    add = rows_of(res).double() if res is not None else None
    e_add = 0.0 if res is not None else None
    if st is None:
        L = chain_stats(M, C, False)
        e_mean, e_var = fwd_stats_bound(x64, L)
        ref, _ = check_fwd(rep, tag, x64, w64, b64, eps, relu, rows_of(y), mean, invstd, e_mean, e_var, add, e_add)
        ref["e_mean"], ref["e_var"] = e_mean, e_var
    else:
        check_partials(rep, tag, st, x64, t)
        mean_t, var_t, e_mean, e_var, L = tiles_stats(st, t, M)
        ref, _ = check_fwd_given(rep, tag, x64, w64, b64, eps, relu, rows_of(y), mean, invstd, mean_t, var_t, e_mean, e_var,
                                 add, e_add)
    assert L <= L_MAX
    if rm is not None:
        check_running(rep, tag, rm, rv, init[rm.data_ptr()].double(), init[rv.data_ptr()].double(), ref, M, bk.f32(mom))
    ypos = rows_of(y) > 0
    assert (mask is not None) == (relu and res is not None)
    if mask is not None:
        rep.exact(tag + "mask", torch.equal(unpack_mask(mask, M, C), ypos))
    return ypos


def audit_pair_forward(rep, tag, call, init):
    """One observed bn_act_fwd_tiles_bnres call, by the checks of test_bn_pair from the observed partials."""
    (x, st, t, w, b, rm, rv, eps, mom, r, rst, rt, rw, rb, rrm, rrv, reps, rmom, _), _, out = call
    w, b, rw, rb = (t_.detach() for t_ in (w, b, rw, rb))
    y, mean, invstd, mask, rmean, rinvstd = out
    C = x.shape[1]
    x64, r64 = rows_of(x).double(), rows_of(r).double()
    M = x64.shape[0]
    eps, reps = bk.f32(eps), bk.f32(reps)
    check_partials(rep, tag, st, x64, t)
    check_partials(rep, tag + "r ", rst, r64, rt)
    mean_t, var_t, e_mean, e_var, L = tiles_stats(st, t, M)
    rmean_t, rvar_t, re_mean, re_var, rL = tiles_stats(rst, rt, M)
    assert max(L, rL) <= L_MAX
    rinv = (rvar_t + reps) ** -0.5
    rpre = (r64 - rmean_t) * rinv * rw.double() + rb.double()
    re_inv = bk.invstd_bound(rvar_t, reps, re_var)
    re_v = bk.preact_bound(r64, rmean_t, rinv, rw.double(), rb.double(), re_mean, re_inv)
    ref, _ = check_fwd_given(rep, tag, x64, w.double(), b.double(), eps, True, rows_of(y), mean, invstd, mean_t, var_t,
                             e_mean, e_var, rpre, re_v)
    rep.add(tag + "rmean", rmean, rmean_t, re_mean)
    rep.add(tag + "rinvstd", rinvstd, rinv, re_inv)
    rref = dict(mean=rmean_t, var=rvar_t, e_mean=re_mean, e_var=re_var)
    check_running(rep, tag, rm, rv, init[rm.data_ptr()].double(), init[rv.data_ptr()].double(), ref, M, bk.f32(mom))
    check_running(rep, tag + "r ", rrm, rrv, init[rrm.data_ptr()].double(), init[rrv.data_ptr()].double(), rref, M,
                  bk.f32(rmom))
    ypos = rows_of(y) > 0
    rep.exact(tag + "mask", torch.equal(unpack_mask(mask, M, C), ypos))
    return ypos


def audit_bn_backward(rep, tag, rec, gmask, part=None, rlink=False):
    """A tapped _BNActFn node's backward by check_bwd: g = (the dy it received) (.) gmask (None: no ReLU), the
    saved x, mean and invstd.  part: the conv_dgrad_bn partial rows it took through its link.  rlink: its
    residual gradient is handed on unmasked and must be the dy tensor itself."""
    x, _, mean, invstd, w, _ = (None if t is None else t.detach() for t in rec["saved"])
    fn, gi, dy = rec["fn"], rec["gi"], rec["go"][0]
    g = rows_of(dy).double()
    if gmask is not None:
        g = g * gmask
    x64 = rows_of(x).double()
    M, C = x64.shape
    xc = x64 - mean.double()
    if part is not None:
        L = LT + chain_rows(part.shape[0], True)
        sums = (g.sum(0), (g * xc).sum(0), L * U * g.abs().sum(0), (L + 2) * U * (g * xc).abs().sum(0))
    else:
        L = chain_stats(M, C, True)
        sums = bk.bwd_sums(g, xc, L, exact_s1=False)
    assert L <= L_MAX
    want_dres = fn.has_res and not rlink
    out = (gi[0], gi[3] if want_dres else None, gi[1], gi[2])
    check_bwd(rep, tag, out, g, x64, mean, invstd, w.detach().double(), L, want_dres, sums=sums)
    if fn.has_res and rlink:
        rep.exact(tag + "dres is dy", gi[3].data_ptr() == dy.data_ptr() and same_bits(gi[3], dy))
    return g


def audit_pair_backward(rep, tag, rec, ypos):
    """A tapped _BNActBNResFn node's backward: both BatchNorms from the shared g = dy (.) ypos (test_bn_pair)."""
    x, r, _, mean, invstd, w, _, rmean, rinvstd, rw, _ = (t.detach() for t in rec["saved"])
    gi = rec["gi"]
    g = rows_of(rec["go"][0]).double() * ypos
    M, C = g.shape
    Lb = chain_stats(M, C, True)
    assert Lb <= L_MAX
    for side, xx, mu, iv, ww, o in (("x ", x, mean, invstd, w, gi[0:3]), ("r ", r, rmean, rinvstd, rw, gi[3:6])):
        x64, mu64, iv64, w64 = rows_of(xx).double(), mu.double(), iv.double(), ww.detach().double()
        xc = x64 - mu64
        s1, s2, e_s1, e_s2 = bk.bwd_sums(g, xc, Lb, exact_s1=False)
        dx_ref, dg_ref, db_ref = bn_bwd_ref(g, x64, mu64, iv64, w64)
        e_dx, e_dg, e_db = bk.bwd_bound(s1, s2, e_s1, e_s2, g, xc, iv64, w64, M)
        rep.add(tag + side + "dx", rows_of(o[0]), dx_ref, out_bound(dx_ref, e_dx))
        rep.add(tag + side + "dgamma", o[1], dg_ref, e_dg)
        rep.add(tag + side + "dbeta", o[2], db_ref, e_db)


def conv_grads64(x, w, dy, stride):
    """float64 dX, dW of conv(x, w) for dy on the CPU, and the same sums over absolute values (the terms)."""
    x, w, dy = (t.detach().double().cpu() for t in (x, w, dy))
    pad = (w.shape[-1] - 1) // 2
    out = []
    for xx, ww, dd in ((x, w, dy), (x.abs(), w.abs(), dy.abs())):
        xr, wr = xx.clone().requires_grad_(), ww.clone().requires_grad_()
        out.extend(torch.autograd.grad(F.conv2d(xr, wr, stride=stride, padding=pad), (xr, wr), dd))
    return out


def audit_conv(rep, tag, rec, y_obs, add=None, cadd=None):
    """A tapped _ConvFn node: y, dX and dW inside K 2^-24 sum |terms| plus the output's half spacing.  add:
    the (masked) joining gradient in conv1's dX; cadd: the observed compact gradient added at (2a, 2b)."""
    R_, m = _R(), _m()
    x, wb = rec["saved"]
    fn, gi, dy = rec["fn"], rec["gi"], rec["go"][0]
    K, C, R, _ = wb.shape
    N, _, H, W = x.shape
    st, T = fn.stride, N * H * W
    ref, e = conv_bound(x, wb, st, R * R * C)
    rep.add(tag + "y", y_obs.detach().cpu(), ref, out_bound(ref, e))
    p, dw, pt, dwt = conv_grads64(x, wb, dy, st)
    one = R == 1 and st == 1
    if gi[0] is not None:
        e_p = R * R * K * U * pt
        ref_dx, bound = p, out_bound(p, e_p)
        if add is not None:
            ref_dx = p + add.detach().double().cpu()
            single = not (one and R_._gemm_dgrad_1x1(m, T, C, K)) or nt4(K)
            bound = out_bound(ref_dx, e_p) if single else out_bound(ref_dx, out_bound(p, e_p))
        if cadd is not None:
            px = torch.zeros(H, W, dtype=torch.bool)
            px[::2, ::2] = True
            ref2 = ref_dx + zero_fill(cadd.detach().double().cpu(), H, W)
            bound = torch.where(px, out_bound(ref2, bound), bound)
            ref_dx = ref2
        rep.add(tag + "dx", gi[0].cpu(), ref_dx, bound)
    e_w = (dy.numel() // K) * U * dwt
    dw_gemm = one and R_._gemm_wgrad_1x1(C, K) and (dy.numel() // K) % 64 == 0
    rep.add(tag + "dw", gi[1].cpu(), dw, out_bound(dw, e_w) if dw_gemm else e_w + U * dw.abs())
    return p, pt


BLOCKS = {  # cin, width, stride, downsample channels or None, input shape
    "ident-T256": (256, 64, 1, None, (4, 256, 8, 8)),
    "ident-T147": (256, 64, 1, None, (3, 256, 7, 7)),
    "ident-wide-T256": (1024, 256, 1, None, (4, 1024, 8, 8)),
    "ds2-16x32": (256, 128, 2, 512, (2, 256, 16, 32)),
    "ds2-14x14": (256, 128, 2, 512, (3, 256, 14, 14)),
    "ds1-T256": (64, 64, 1, 256, (4, 64, 8, 8)),
}
BLOCK_CASES = [
    ("ident-T256", {}), ("ident-T256", dict(_BN_LINK=False)), ("ident-T256", dict(_RES_MASK=False)),
    ("ident-T256", dict(_GEMM_BN_STATS=False)),
    ("ident-T147", {}), ("ident-T147", dict(_RES_MASK=False)),
    ("ident-wide-T256", {}),
    ("ds2-16x32", {}), ("ds2-16x32", dict(_DS_FUSED=False)), ("ds2-16x32", dict(_DS_FUSED=False, _RES_MASK=False)),
    ("ds2-16x32", dict(_DS_COMPACT=False)), ("ds2-16x32", dict(_BN_LINK=False, _DS_COMPACT=False)),
    ("ds2-14x14", {}), ("ds2-14x14", dict(_DS_FUSED=False)),
    ("ds1-T256", {}), ("ds1-T256", dict(_DS_FUSED=False)),
]


def case_id(case):
    kind, hk = case
    return kind + "".join(f"-{k.strip('_').lower()}={int(v)}" for k, v in hk.items())


def make_block(kind, seed=5):
    from paddle_operator_amd.models.resnet import Bottleneck
    cin, width, stride, dsk, _ = BLOCKS[kind]
    torch.manual_seed(seed)
    ds = None
    if dsk is not None:
        ds = torch.nn.Sequential(torch.nn.Conv2d(cin, dsk, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(dsk))
    blk = Bottleneck(cin, width, stride=stride, downsample=ds)
    for mod in blk.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(mod.weight, 0.5, 1.5)
            torch.nn.init.uniform_(mod.bias, -0.2, 0.2)
            torch.nn.init.normal_(mod.running_mean, 0.0, 0.1)
            torch.nn.init.uniform_(mod.running_var, 0.5, 1.5)
    return blk.cuda().to(memory_format=torch.channels_last)


def expected_links(kind, hk, m=None):
    """(_BN_LINK_USED, _RES_MASK_USED, _DS_COMPACT_USED) one forward and backward of the block must move."""
    R, m = _R(), (_m() if m is None else m)
    cin, width, stride, dsk, (N, _, H, W) = BLOCKS[kind]
    on = lambda k: hk.get(k, True)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gemm3 = bool(R._gemm_dgrad_1x1(m, N * Ho * Wo, width, 4 * width))
    bn = (1 + (0 if gemm3 else 1)) if on("_BN_LINK") else 0
    res = int(on("_RES_MASK") and (dsk is None or not on("_DS_FUSED")))
    ds = int(dsk is not None and stride == 2 and on("_DS_COMPACT") and bool(m.gemm_nt_supported(N * Ho * Wo, cin, dsk)))
    return (bn, res, ds)


def run_block(blk, kind, hk, retain=False):
    m = _m()
    shape = BLOCKS[kind][4]
    x = dev_cl(rand_bf16(shape, 71)).requires_grad_()
    init = {b.data_ptr(): b.detach().clone() for b in blk.buffers() if b.dtype.is_floating_point}
    with hooks(**hk), links() as lk, capture(m, *CAPTURE) as log, torch.autocast("cuda", dtype=BF16):
        y = blk(x)
        names = nodes(y)
        recs = tap(y)
        dy = dev_cl(rand_bf16(tuple(y.shape), 72))
        y.backward(dy, retain_graph=retain)
        torch.cuda.synchronize()
    return dict(x=x, y=y, dy=dy, names=names, recs=recs, log=log, used=lk.used, init=init)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=case_id)
def test_bottleneck_nodes_per_element(cuda, case):
    """Every node of a Bottleneck under one route combination against the float64 of that node alone, from
    its observed inputs; the route by node classes and link counters; the link contracts bit for bit."""
    kind, hk = case
    cin, width, stride, dsk, shape = BLOCKS[kind]
    blk = make_block(kind)
    r = run_block(blk, kind, hk)
    recs, log = r["recs"], r["log"]
    want_links = expected_links(kind, hk)
    assert r["used"] == want_links, f"{case_id(case)}: link counters moved by {r['used']}, expected {want_links}"
    fused_tail = dsk is not None and hk.get("_DS_FUSED", True)
    assert route_ok(r["names"], ["_ConvFn", "_BNActFn"] + (["_BNActBNResFn"] if fused_tail else []),
                    [] if fused_tail else ["_BNActBNResFn"]), sorted(r["names"])
    assert len(log["bn_act_bwd_part"]) == want_links[0] and len(log["conv_stride2_add"]) == want_links[2]
    rep = Report(f"block {case_id(case)}")
    convs = {n: mod for n, mod in (("conv1", blk.conv1), ("conv2", blk.conv2), ("conv3", blk.conv3))}
    bns = {"bn1": blk.bn1, "bn2": blk.bn2}
    if dsk is not None:
        convs["ds"] = blk.downsample[0]
    if not fused_tail:
        bns["bn3"] = blk.bn3
        if dsk is not None:
            bns["dsbn"] = blk.downsample[1]
    cv = {n: next(q for q in of_class(recs, "_ConvFn") if q["fn"].wparam is mod.weight) for n, mod in convs.items()}
    bn = {n: next(q for q in of_class(recs, "_BNActFn") if q["fn"].params[0] is mod.weight) for n, mod in bns.items()}
    assert len(of_class(recs, "_ConvFn")) == len(cv) and len(of_class(recs, "_BNActFn")) == len(bn)
    assert all(q["runs"] == 1 for q in recs)
    # ---- forward: every BatchNorm from its observed call
    fwd = {c[0][0].data_ptr(): (c, False) for c in log["bn_act_fwd"]}
    fwd.update({c[0][0].data_ptr(): (c, True) for c in log["bn_act_fwd_tiles"]})
    stats_pass = {n for n in bn if not fwd[bn[n]["saved"][0].data_ptr()][1]}
    assert stats_pass == ({"bn3"} if hk.get("_GEMM_BN_STATS", True) is False else set()), stats_pass
    ypos = {n: audit_bn_forward(rep, n + " ", *fwd[q["saved"][0].data_ptr()], r["init"]) for n, q in bn.items()}
    if fused_tail:
        pair = of_class(recs, "_BNActBNResFn")[0]
        ypos["pair"] = audit_pair_forward(rep, "tail ", log["bn_act_fwd_tiles_bnres"][0], r["init"])
    # ---- the BatchNorm backward passes and the link contracts
    parts = {c[0][3].data_ptr(): c[0][0] for c in log["bn_act_bwd_part"]}
    res_mask = hk.get("_RES_MASK", True)
    for n in ("bn1", "bn2"):
        audit_bn_backward(rep, n + " ", bn[n], ypos[n], part=parts.get(bn[n]["saved"][0].data_ptr()))
    if fused_tail:
        audit_pair_backward(rep, "tail ", pair, ypos["pair"])
    else:
        audit_bn_backward(rep, "bn3 ", bn["bn3"], ypos["bn3"], rlink=res_mask)
        assert same_bits(bn["bn3"]["go"][0], r["dy"])
        if dsk is not None:
            # mlink: the downsample BatchNorm receives bn3's dy unmasked and applies bn3's mask itself
            d = bn["dsbn"]
            rep.exact("dsbn dy", same_bits(d["go"][0], bn["bn3"]["gi"][3]))
            audit_bn_backward(rep, "dsbn ", d, ypos["bn3"] if res_mask else None)
    # ---- the convolutions
    outs = {"conv1": bn["bn1"]["saved"][0], "conv2": bn["bn2"]["saved"][0]}
    if fused_tail:
        outs["conv3"], outs["ds"] = pair["saved"][0], pair["saved"][1]
    else:
        outs["conv3"] = bn["bn3"]["saved"][0]
        if dsk is not None:
            outs["ds"] = bn["dsbn"]["saved"][0]
    for n in ("conv2", "conv3"):
        audit_conv(rep, n + " ", cv[n], outs[n])
    c1, add, cadd = cv["conv1"], None, None
    dal = c1["go"][2]
    if dsk is None:
        b3 = bn["bn3"]
        rep.exact("conv1 dalias is bn3's dres", dal.data_ptr() == b3["gi"][3].data_ptr() and same_bits(dal, b3["gi"][3]))
        N, C, H, W = shape
        keep = ypos["bn3"].view(N, H, W, C).permute(0, 3, 1, 2)
        # with the link the mask appears only here: dalias is bn3's dy unmasked
        add = dal.double() * keep if res_mask else dal.double()
        if not res_mask:
            rep.exact("bn3 dres masked", bool(((dal != 0) <= keep).all()))
    else:
        d = cv["ds"]
        if want_links[2]:
            rep.exact("compact: no downsample dX, no dalias", d["gi"][0] is None and dal is None)
            cadd = log["conv_stride2_add"][0][0][1]
            pds, pdt = audit_conv(rep, "ds ", d, outs["ds"])
            Kd = dsk
            rep.add("ds compact dx", cadd.cpu(), pds[:, :, ::2, ::2], out_bound(pds, Kd * U * pdt)[:, :, ::2, ::2])
        else:
            audit_conv(rep, "ds ", d, outs["ds"])
            rep.exact("conv1 dalias is the downsample's dX", same_bits(dal, d["gi"][0]))
            add = dal.double()
    audit_conv(rep, "conv1 ", c1, outs["conv1"], add=add, cadd=cadd)
    rep.exact("conv1 dx is x.grad", same_bits(c1["gi"][0], r["x"].grad))
    rep.check()


# ---------------------------------------------------------------------------------------------
# (b) the stem
# ---------------------------------------------------------------------------------------------
STEM_ROUTES = {
    "fused": ({}, ["_StemFn", "_BNReluPoolFn"], ["_BNActFn", "_MaxPool3s2Fn"]),
    "unfused": (dict(_STEM_POOL=False), ["_StemFn", "_BNActFn", "_MaxPool3s2Fn"], ["_BNReluPoolFn"]),
    "framework": (dict(_HIP_STEM=False), ["_BNActFn", "_MaxPool3s2Fn"], ["_StemFn", "_BNReluPoolFn"]),
}


@pytest.mark.parametrize("name", list(STEM_ROUTES))
def test_stem_nodes_per_element(cuda, name):
    """The stem on its three routes (N 2, a 16 x 24 image): node classes, and every node against float64 of
    its observed inputs — the 7 x 7 convolution and its weight gradient inside K 2^-24 sum |terms|, the
    BatchNorm from the observed tile statistics, the pool's choice of the first maximum, dx by the scatter
    reference; check_stem itself on the observed stem output."""
    ops, m = _ops(), _m()
    hk, ran, not_ran = STEM_ROUTES[name]
    N, H, W = 2, 16, 24
    torch.manual_seed(9)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(10)
    bn = bn_module(64, 0.5 + torch.rand(64, generator=g), 0.2 * torch.randn(64, generator=g))
    init = {b.data_ptr(): b.detach().clone() for b in bn.buffers() if b.dtype.is_floating_point}
    xv = rand_bf16((N, 3, H, W), 81)
    x = dev_cl(xv)
    with hooks(**hk), links() as lk, capture(m, *CAPTURE) as log, torch.autocast("cuda", dtype=BF16):
        y = ops.conv_bn_relu_maxpool(conv, bn, x)
        assert_route(y, ran, not_ran)
        recs = tap(y)
        dyv = ints(tuple(y.shape), 4, 82)
        y.backward(cx.dev_bf16(dyv))
        torch.cuda.synchronize()
    assert lk.used == (0, 0, 0)
    rep = Report(f"stem {name}")
    wb = conv.weight.detach().to(BF16)
    OH, OW = H // 2, W // 2
    if name == "fused":
        node = of_class(recs, "_BNReluPoolFn")[0]
        xs, yp, xsel, arg, mean, invstd, w, b = node["saved"]
        (a, _, (_, st, _)), = log["stem_fwd"]
        t, M = m.stem_tile_rows(), N * OH * OW
        w, b = w.detach(), b.detach()
        x64, w64, b64 = rows_of(xs).double(), w.double(), b.double()
        check_partials(rep, "", st, x64, t)
        mean_t, var_t, e_mean, e_var, L = tiles_stats(st, t, M)
        inv = (var_t + EPS) ** -0.5
        e_inv = bk.invstd_bound(var_t, EPS, e_var)
        rep.add("mean", mean, mean_t, e_mean)
        rep.add("invstd", invstd, inv, e_inv)
        ref = dict(mean=mean_t, var=var_t, e_mean=e_mean, e_var=e_var)
        check_running(rep, "", bn.running_mean, bn.running_var, init[bn.running_mean.data_ptr()].double(),
                      init[bn.running_var.data_ptr()].double(), ref, M, MOM)
        PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
        arg4 = arg.view(N, PH, PW, 64)
        x4 = rows_of(xs).view(N, OH, OW, 64)
        rep.exact("xsel = x[arg]", same_bits(rows_of(xsel).view(N, PH, PW, 64), bk.pool_gather(x4, arg4)))
        act = ((x64 - mean_t) * inv * w64 + b64).clamp_min(0.0).view(N, OH, OW, 64)
        e_v = bk.preact_bound(x64, mean_t, inv, w64, b64, e_mean, e_inv).view(N, OH, OW, 64)
        bound = out_bound(act, e_v)
        ysel = rows_of(yp).view(N, PH, PW, 64)
        rep.add("y", ysel, bk.pool_gather(act, arg4), bk.pool_gather(bound, arg4))
        below = max(float(((a_p - ysel.double()) / b_p)[~torch.isnan(x_p)].max()) for a_p, b_p, x_p in
                    zip(bk.pool_windows(act, -float("inf")), bk.pool_windows(bound, 1.0), bk.pool_windows(x4.double(), float("nan"))))
        rep.rows.append(("window <= y", max(below, 0.0)))
        # backward: dy scattered to the chosen positions, the ReLU mask from the forward's own y
        mu, iv = mean.double(), invstd.double()
        dy = cx.dev_bf16(dyv)
        gp = rows_of(dy).double() * (ysel.reshape(-1, 64) > 0)
        gfull = bk.pool_scatter(gp.view(N, PH, PW, 64), arg4, OH, OW).reshape(M, 64)
        Lb = chain_stats(N * PH * PW, 64, True)
        xc = x64 - mu
        s1, s2, e_s1, e_s2 = bk.bwd_sums(gp, rows_of(xsel).double() - mu, Lb)
        dx_ref, dg_ref, db_ref = bn_bwd_ref(gfull, x64, mu, iv, w64)
        e_dx, e_dg, _ = bk.bwd_bound(s1, s2, e_s1, e_s2, gfull, xc, iv, w64, M)
        rep.add("dx", rows_of(node["gi"][0]), dx_ref, out_bound(dx_ref, e_dx))
        rep.add("dgamma", node["gi"][1], dg_ref, e_dg)
        rep.exact("dbeta exact", torch.equal(node["gi"][2].double(), db_ref))
        assert max(L, Lb) <= L_MAX
        # the kernels' own check on the same observed stem output (its own 7-row partials)
        check_stem(m, cuda, N, 64, OH, OW, rows_of(xs).contiguous(), w, b, rows_of(dy).contiguous(),
                   init[bn.running_mean.data_ptr()], init[bn.running_var.data_ptr()], rep)
        stem_y, stem_dy = xs, node["gi"][0]
    else:
        node = of_class(recs, "_BNActFn")[0]
        pool = of_class(recs, "_MaxPool3s2Fn")[0]
        calls_ = log["bn_act_fwd_tiles"] if name == "unfused" else log["bn_act_fwd"]
        ypos = audit_bn_forward(rep, "bn ", calls_[0], name == "unfused", init)
        audit_bn_backward(rep, "bn ", node, ypos)
        ybn = calls_[0][2][0]
        a4 = rows_of(ybn).view(N, OH, OW, 64)
        best, arg_ref = bk.pool_fwd_ref(a4)
        rep.exact("pool y", same_bits(rows_of(y.detach()).view(best.shape), best))
        sc = bk.pool_scatter(rows_of(cx.dev_bf16(dyv)).double().view(best.shape), arg_ref, OH, OW)
        rep.exact("pool dx", bool((rows_of(pool["gi"][0]).view(sc.shape).double() == sc.to(BF16).double()).all()))
        assert float(sc.abs().max()) <= 256     # sums of at most 4 integers in [-4, 4]: exact in bf16
        rep.exact("pool dx is the BatchNorm's dy", same_bits(pool["gi"][0], node["go"][0]))
        stem_y, stem_dy = node["saved"][0], node["gi"][0]
    if name == "framework":      # (the framework convolution's rounding is not the project's to state)
        rep.check()
        return
    # _StemFn: y and dW against float64
    xc64, wc64 = xv.double(), wb.double().cpu()
    ref = F.conv2d(xc64, wc64, stride=2, padding=3)
    e = 147 * U * F.conv2d(xc64.abs(), wc64.abs(), stride=2, padding=3)
    rep.add("conv y", stem_y.detach().cpu(), ref, out_bound(ref, e))
    wr = wc64.clone().requires_grad_()
    dw, = torch.autograd.grad(F.conv2d(xc64, wr, stride=2, padding=3), (wr,), stem_dy.detach().double().cpu())
    wa = wc64.abs().requires_grad_()
    dwt, = torch.autograd.grad(F.conv2d(xc64.abs(), wa, stride=2, padding=3), (wa,), stem_dy.detach().double().cpu().abs())
    rep.add("conv dw", conv.weight.grad.detach().cpu(), dw, N * OH * OW * U * dwt + U * dw.abs())
    rep.check()


# ---------------------------------------------------------------------------------------------
# (c) identity and failure behaviour of the hand-offs inside whole blocks
# ---------------------------------------------------------------------------------------------
def block_grads(blk, x):
    return dict(x=x.grad.detach().clone(), **{n: p.grad.detach().clone() for n, p in blk.named_parameters()})


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for n in a:
        assert same_bits(a[n], b[n]), f"{what}: {n} differs"


@pytest.mark.parametrize("kind", ("ident-T256", "ds2-16x32"))
def test_shadow_weights_bit_identical(cuda, kind):
    """The arena's bf16 shadow and its batched W^T against one cast per forward and one transpose per
    backward: copies of the same bits, so every output is bit-identical; which one ran shows in the
    conv_weight_t / transpose calls."""
    from paddle_operator_amd.parallel.flat import FlatParams
    m = _m()
    blk = make_block(kind)
    flat = FlatParams(blk, dtype=torch.float32, device="cuda")
    flat.enable_shadow()
    res, n_t = {}, {}
    for mode in ("cast", "shadow", "shadow-no-wt"):
        if mode == "shadow-no-wt":
            for p in blk.parameters():
                if hasattr(p, "_pdo_shadow_t"):
                    del p._pdo_shadow_t
        flat.zero_grad()
        scope = flat.shadow_scope() if mode != "cast" else contextlib.nullcontext()
        with scope, calls(m, "conv_weight_t", "transpose") as n:
            r = run_block(blk, kind, {})
        assert r["used"] == expected_links(kind, {})
        res[mode] = dict(y=r["y"].detach().clone(), **block_grads(blk, r["x"]))
        n_t[mode] = n["conv_weight_t"] + n["transpose"]
    assert n_t["shadow"] == 0 and n_t["cast"] == n_t["shadow-no-wt"] > 0, n_t
    assert_same(res["cast"], res["shadow"], f"{kind}: shadow weights")
    assert_same(res["cast"], res["shadow-no-wt"], f"{kind}: shadow weights, per-backward transpose")


@pytest.mark.parametrize("kind", ("ident-T256", "ds2-16x32", "ident-wide-T256"))
def test_arena_route_matches_returned_route(cuda, kind):
    """Gradients written straight into a zeroed fp32 arena against the returned-gradient route: dX and every
    BatchNorm dx bit-identical, every parameter gradient equal after the fp32 add onto zero."""
    import copy

    from paddle_operator_amd.parallel.flat import FlatParams
    a = make_block(kind)
    b = copy.deepcopy(a)
    flat = FlatParams(a, dtype=torch.float32, device="cuda")
    flat.zero_grad()
    ra, rb = run_block(a, kind, {}), run_block(b, kind, {})
    assert ra["used"] == rb["used"] == expected_links(kind, {})
    for p in a.parameters():
        assert flat.grads.data_ptr() <= p.grad.data_ptr() < flat.grads.data_ptr() + flat.grads.numel() * 4
    assert_same(dict(y=ra["y"], **block_grads(a, ra["x"])), dict(y=rb["y"], **block_grads(b, rb["x"])), f"{kind}: arena")
    for qa, qb in zip(ra["recs"], rb["recs"]):
        assert qa["cls"] == qb["cls"]
        if qa["gi"][0] is None:      # the compact downsample convolution returns no input gradient
            assert qb["gi"][0] is None
        else:
            assert same_bits(qa["gi"][0], qb["gi"][0]), f"{kind}: {qa['cls']} dx differs"
        if qa["cls"] == "_ConvFn":   # (no convolution of these blocks takes gemm_dw, whose dW is returned)
            assert qa["gi"][1] is None and qb["gi"][1] is not None, "dW written in place / returned"


ALL_OFF = dict(_BN_LINK=False, _RES_MASK=False, _DS_COMPACT=False)


@pytest.mark.parametrize("kind,hk", [("ident-T256", {}), ("ident-T147", {}), ("ds2-16x32", {}), ("ds2-16x32", dict(_DS_FUSED=False))],
                         ids=["ident-T256", "ident-T147", "ds2-fused", "ds2-two-pass"])
def test_second_backward_through_retained_graph(cuda, kind, hk):
    """Every link is consumed by the first backward; a second backward through the retained graph moves no
    counter and has the bits of a first backward with the links switched off (the same kernels on the same
    bits: conv_dgrad for conv_dgrad_bn, the BatchNorm's own masked dres, the zero-filled downsample dX)."""
    import copy
    a = make_block(kind)
    b = copy.deepcopy(a)
    r = run_block(a, kind, hk, retain=True)
    assert r["used"] == expected_links(kind, hk)
    first = block_grads(a, r["x"])
    r["x"].grad = None
    for p in a.parameters():
        p.grad = None
    with hooks(**hk), links() as lk:
        r["y"].backward(r["dy"])
        torch.cuda.synchronize()
    assert lk.used == (0, 0, 0)
    second = block_grads(a, r["x"])
    off = dict(hk, **ALL_OFF)
    rb = run_block(b, kind, off)
    assert rb["used"] == (0, 0, 0)
    assert_same(second, block_grads(b, rb["x"]), f"{kind} {hk}: second backward against the links-off backward")
    assert same_bits(r["y"], rb["y"])
    # (the first backward took the links: its bands are test_bottleneck_nodes_per_element's)
    assert first.keys() == second.keys()


@pytest.mark.parametrize("kind,hk", [("ident-T256", {}), ("ds2-16x32", dict(_DS_FUSED=False))], ids=["ident", "ds2-two-pass"])
def test_no_grad_forward_matches_and_creates_no_link(cuda, kind, hk):
    """A torch.no_grad() forward with bn.training: no link objects, y and the running statistics with the bits
    of the grad-enabled forward."""
    ops = _ops()
    a, b, c = (make_block(kind) for _ in range(3))     # the same seed: the same parameters and buffers
    x = dev_cl(rand_bf16(BLOCKS[kind][4], 71))
    with hooks(**hk), torch.autocast("cuda", dtype=BF16):
        ya = a(x.clone().requires_grad_())
        with torch.no_grad(), links() as lk:
            yb = b(x)
            out, xa = ops.conv_bn_act(c.conv1, c.bn1, x, fork=True)
    assert lk.used == (0, 0, 0) and not yb.requires_grad
    for t in (out, xa):
        assert all(getattr(t, k, None) is None for k in ("_pdo_bn", "_pdo_rlink", "_pdo_slink"))
    assert same_bits(ya.detach(), yb)
    for (n, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        assert p.dtype != torch.float32 or same_bits(p, q), f"running statistic {n} differs under no_grad"
        if n.endswith("running_var"):
            assert not same_bits(p, dict(c.named_buffers())[n]) or n.startswith("bn1")   # (and it was updated)
