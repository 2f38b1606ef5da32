"""Bit-exact and per-element float64 checks of the GPT-2 autograd nodes and their routes
(paddle_operator_amd/ops/gpt2.py, ops/core.py): the layer that wires the HIP kernels into a training
step.  The kernels themselves are held to their rounding contracts by test_gemm_nt_exact_gpu.py,
test_gemm_dw_exact_gpu.py, test_ln_gelu_embed_gpu.py, test_attention_exact_gpu.py and
test_small_kernels_gpu.py; this file imports their builders and checkers and applies them one level
up, where a norm over a whole tensor cannot see a dropped row, a gradient handed to the wrong input,
a wrong `accumulate` or a bias added twice.  test_gpt2_nodes_cpu.py validates the builders and
references below and shows the checkers rejecting each of those mistakes.

Route table.  Every case asserts the autograd node classes that ran (nodes(): the class names reachable
from grad_fn through next_functions); a case whose route was not taken fails.  Hooks are one-element
lists of ops.core / ops.gpt2, set by hooks() inside try / finally.  C = 256, 4 heads of 64, hidden
1024; T = 256 is one tile row, T = 768 three (the XCD remap then has a remainder).

    op                     route (node classes)                 selected by                        forced by            smallest shape
    linear                 _LinearFn on gemm_nt4 / gemm_dw      M % 256 == 0, K % 128 == 0, >= 256 default              T 256, C 256
                           _LinearFn on the 8-wave ring         K < 256                            shape                C 128
                           _LinearFn on the library             M % 256 != 0                       shape, _NT_ALL = 0   T 192
                           dX = dy @ W (library)                                                   _DX_TN = False       T 256
                           dW on the library (addmm_)           gemm_dw declines (N % 256 != 0)    _HIP_DW = False      C 128
    layer_norm             _LayerNormFn                         always                             -                    T 256
    add_layer_norm         _AddLayerNormFn                      drop is None or thr == 0           -                    T 256
                           _AddLayerNormDropFn                  thr > 0                            drop=                T 256
    layer_norm_res         _LNResFn                             contiguous x, no drop              -                    T 256
                           _LNResDropFn                         drop                               drop=                T 256
                           _LayerNormFn                         non-contiguous x                   a view               T 256
    linear_add_layer_norm  _LinearResFn -> _LNResFn             _res_epi_ok (K >= 256, 4-wave)     _RES_EPI (default)   T 256
                           _LinearFn -> _AddLayerNormFn         else                               _RES_EPI = False,    C 128, T 192
                                                                                                   a view
                           _LinearFn -> _AddLayerNormDropFn     drop                               drop=                T 256
    mlp                    _NTMLPFn, saved gelu' (EPI 7 / 8)    gemm_nt_epi_ok                     _NT_GD (default)     T 256
                           _NTMLPFn, recomputing (EPI 2 / 3)                                       _NT_GD = False       T 256
                           _LinearFn -> _GeluLinearFn           fc1 shape outside the contract     _NT_GELU = False     T 256
                           _LinearFn -> _BiasGeluFn -> _LinearFn  fc2 dX outside the contract      _NT_DGELU = False    T 192
    mlp_add_layer_norm     _NTMLPFn(res) -> _LNResFn            as mlp and _res_epi_ok             default              T 256
                           mlp -> _AddLayerNormFn               else                               _RES_EPI = False     T 256
    bias_gelu              _BiasGeluFn                          always                             (_NT_DGELU = False)  T 256
    qkv_attention          _QKVAttnFn                           head dim 64, S % 128 == 0          _QKV_FUSED (default) S 128
                           _LinearFn -> _FlashAttnFn                                               _QKV_FUSED = False   S 128
                           _LinearFn -> framework SDPA          head dim 32 or S = 96              shape                S 96
    attention              _FlashAttnFn / framework SDPA        as above                           shape                S 128 / 96
    lm_head_xent           _LMHeadXentFn, xent_fused            gemm_nt_supported, N % chunk == 0  _LM_CHUNK = -1, 256  N 512, V 300
                           _LMHeadXentFn, xent_fwd + xent_bwd                                      _XENT_FUSED = False  N 512
                           _lm_head_loss_only                   no_grad                            torch.no_grad()      N 512
                           _LinearFn -> _XentFn                 chunk 0                            _LM_CHUNK = 0        N 512
                           _SplitHeadLinearFn -> _XentFn        chunk 0 and a split weight         _LM_CHUNK = 0        N 512
    cross_entropy          _XentFn                              always                             (_LM_CHUNK = 0)      N 512
    embedding              _EmbedFn, atomic embed_bwd           no split slot                      -                    2 x 384
                           _EmbedFn, embed_bwd_sorted           FlatParams(split=("wte",))         split=               2 x 384
    weight-gradient queue  gemm_dw4_grouped / one launch each   deferred_weight_grads              _DW_GROUPED, _DW_CUS T 256

(a) Bit-exact on dyadic grids.  Operands are those of test_gemm_nt_exact_gpu.py: activations integers
in [-15, 15], weights integers of magnitude 8 .. 15 times 2^-s, biases and the residual stream
integers times 2^-s, incoming gradients integers in [-15, 15]; every fp32 sum is then an integer
(units of 2^-s) below 2^24, asserted per case while it is built, and exact in any order.  Expected
values are float64 products pushed through the contracts stated there: y = RNE(P + b) (EPI 1),
h = RNE((P + b) + x) (EPI 5), dX = RNE(dy W), dW = RNE(base + dy^T a) (gemm_dw with accumulate),
db = RNE(base + sum dy) (colsum with acc).  The unfused residual route rounds twice,
h = RNE(x + RNE(P) + b), and on the grid the two bit patterns differ in a stated share of the
elements (CPU file: at least 5 %).  With the LayerNorm weight set to zero the LayerNorm contributes
exactly zero to dx, so the gradient that enters the producer GEMM equals the integer downstream dh
and the whole chain is exact: dx = dh bit for bit, da, dW, drbias = RNE(sum dh), and with dropout at
p = 0.5 (scale exactly 2) dr = keep 2 dh and drbias = RNE(sum keep 2 dh).  Library routes (F.linear,
addmm_, dy @ W) are held to the same exact product, but where a bias or an accumulate base joins the
product either one rounding or two are accepted: the project does not control that epilogue.

(b) Per-element float64 bands where LayerNorm, GELU or softmax is inside the node.  The reference is
the float64 of that node alone from its stored bf16 inputs; where the node's first kernel has an
exactly known or observable output (h of the epilogue route, the saved qkv, hp and gelu output read
from grad_fn.saved_tensors, x.grad as the residual gradient) that output is used.  Bands are the
constituent kernels' counted bounds through their own checkers: check_ln_forward / ln_bwd_reference
(K_Y, K_B) with check_banded and check_colgrad, check_activation (DELTA = 2^-14) and db_bound for
GELU / GELU', attention's check_forward / check_backward / check_db.  A band is propagated through a
following GEMM as  sum_k band_k |other_k|  +  K 2^-24 sum_k |term_k|  (behind()): dx and dW1 of the
MLP behind the unobservable dhp, dh and dW of the LM head behind the unobservable dlogits.  The band
of a stored bf16 activation output v is DELTA max(|v|, 2^-4) plus half its bf16 spacing; with the
saved-gelu' route dhp = RNE(fl32(P Y)) is known exactly (P exact, Y the stored derivative, one fp32
multiply) and carries no band.  The dlogits band is the rule of test_small_kernels_gpu.py,
2^-8 |ref| + 1e-5 / count; it is a bf16 spacing wide, so the LM-head bands routinely span three bf16
values and WIDE_CAP is not applied there (the share is printed).  A chunked dW adds one bf16 rounding
per chunk after the first (each chunk is RNE(base + sum)): (chunks - 1) 2^-8 sum |term|.

(c) Bit identity between routes that run the same kernels on the same bits, on random data: the
arena route (one backward into a zeroed arena) against the returned-tensor route for every node;
wt_scope live or not (a transpose is a copy); deferred_reductions on or off — colsum_batched runs
colsum_block with the arguments colsum gives it (level 1 over 64-row slices, level 2 over the
partial rows, a job of at most 64 rows finished in level 1), so the order of additions is the same
and the bits are identical; and, on the grid case whose dqkv is no longer on a grid, _QKV_FUSED on or
off (dh and dW identical, db inside check_db's interval).  Routes that run different kernels (_NT_GD, _NT_GELU, _NT_DGELU, _RES_EPI) are each
checked against the float64 reference with their own band.  Grouped against single-launch dW: on the
grid both are RNE(base + exact); _dw_queue.n_grouped moves or does not, and nothing is left queued.
LM head chunk 256 against chunk -1: dh is bit-identical (each row's logits, its dlogits and its dX
are computed by the same GEMMs over the same k order whatever the chunk, and the count is the global
one); dW is not (the per-chunk rounding above) and is checked per element.

Wiring.  Two backwards into one arena with different grid inputs give RNE(RNE(first) + second) for dW
and db of _LinearFn, its library routes and the grouped queue; zero_grad() between them gives the
second alone (every other arena gradient: accum_ok, below).  LM head
targets -100, V, Vp - 1 and -1 among valid ones: their dh rows and dW[V:Vp] are zero, the loss is the
float64 mean over the valid rows, the count is global; dloss = 0.5 gives exactly half of dloss = 1.
A split wte: two forwards then two backwards leave RNE(RNE(d1 dW1) + d2 dW2) in the slot, ready fires
once, after the second; a forward whose graph is dropped leaves the slot's bits untouched.  The
embedding's split route equals sorted_reference onto the gradient's previous bits.  Non-contiguous
inputs (a transposed view, a sliced view) fall to routes that still give the exact product.

dbeta, drbias and the residual producer's dW get the same exact two-backward check on the grid
(test_residual_nodes_exact_chain).  Gradients that are not exact (dgamma, b1, the QKV bias, every
gradient of the random block) are held to accum_ok(): a second micro-batch with other activations and
gradients must leave RNE(first + s2), s2 within half a bf16 spacing of what that micro-batch gives
alone, and zero_grad() followed by it again must give those bits.  Which GEMM path a hook or a scope
selected does not show in the node classes: those cases count the extension calls made (calls()),
and the deferred scope must hold queued column sums before its flush.  The no_grad LM
head allocates less than its logits buffer plus one [Vp, C] buffer at its peak.

Not covered here: the numerics of the framework SDPA fallback (only its route and finiteness).  Where
gemm_dw splits the token axis (T = 512, 768) the per-element dW band carries 2^-8 sum |terms| for the
bf16 partials and spans many bf16 values; those shapes are held mainly by the bit identities and, on
the grid, by the sparse gradients whose dW stays exact.

Measured on an MI355X (each test prints its figures; 55 tests, 5.7 s, the slowest 1.0 s, the first to
touch the device).  Every bit-exact and bit-identity check holds; no check exposed a defect in an op
or a kernel.  Worst error as a share of the counted bound: LayerNorm inside the residual nodes mean
0.000 (the rows are sums on the grid), rstd 0.13 - 0.18, dgamma / dbeta / drbias 0.000 beyond the
output's own rounding; db1 of the MLP 0.81 - 0.92 (db_bound includes that rounding); attention o 0.17,
lse 0.18, dq 0.77, dk 0.24, dv 0.23, the fused QKV bias gradient 0.11.  Band shares: y and dx of the
residual nodes reach a rounding midpoint in 0.35 - 0.54 % of the elements and span more than two values
in at most 0.04 % (WIDE_CAP 0.5 %); the stored gelu / gelu' lie in the ambiguity band in 3.5 - 4.2 %,
47 of 262144 stored gelu' values are the other neighbour.  The propagated GEMM bands are wider by
construction (K 2^-24 sum |terms| against a result of about sum |terms| / sqrt(K)): out and dx of the
MLP span more than two values in 23 - 24 % of the elements at one split, the LM head's dh in 99 % (the
dlogits rule is a bf16 spacing wide), and every dW whose GEMM splits the token axis in all of them.
Grid shares (CPU file): the fused and unfused residual h differ in 26.6 %, y with one and two roundings
in 24.1 %, the fused and unfused gelu outputs in 27.4 %.  LM head: loss 6.007025 against 6.007025 in
float64 over 507 valid targets; chunk 256 gives chunk -1's dh bit for bit and a dW that differs in
17742 of 98304 elements; the no_grad route peaks at 398848 bytes against 393216 of logits.
"""
import contextlib
import functools

import pytest
import torch

import test_attention_exact_gpu as ax
import test_gemm_nt_exact_gpu as ng
import test_ln_gelu_embed_gpu as lg
from test_gemm_dw_exact_gpu import check_bits, same_bits
from test_gemm_nt_exact_gpu import (A_MAX, B_MAG, BAND_FLOOR, DELTA, LIM, _quantum, as_bf16, check_activation, db_bound,
                                    gelu_grad64, rne)
from test_ln_gelu_embed_gpu import (EPS, HO, U, WIDE_CAP, check_banded, check_colgrad, check_ln_forward, interval_ok,
                                    ln_bwd_reference, ln_reference, q16, randn16, sorted_reference)
from test_small_kernels_gpu import xent_ref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
C, HEADS, HID = 256, 4, 1024
S_OF_K = {128: 10, 256: 11, 384: 11, 1024: 12}   # the weight grid 2^-s per contraction length
G_MAX = 15                                      # incoming gradients: integers in [-G_MAX, G_MAX]
SPARSE_NNZ = 16                                 # non-zeros per column of a gradient whose dW is split (grad_ints)
V, VP, LM_N = 300, 384, 512
XENT_REL, XENT_ABS = 2.0 ** -8, 1e-5            # the dlogits rule of test_small_kernels_gpu.py
LOSS_REL = 1e-3                                 # its loss rule: |loss - ref| <= 1e-3 max(1, ref)


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _ops():
    from paddle_operator_amd import ops
    return ops


def record(line):
    print(f"[nodes] {line}")


# ---------------------------------------------------------------------------------------------
# routes and hooks
# ---------------------------------------------------------------------------------------------
def nodes(*tensors):
    """The class names of every autograd node reachable from the tensors' grad_fn."""
    seen, names, stack = set(), set(), [t.grad_fn for t in tensors]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


def route_ok(names, ran, not_ran=()):
    return all(n + "Backward" in names for n in ran) and not any(n + "Backward" in names for n in not_ran)


def assert_route(t, ran, not_ran=()):
    names = nodes(*t) if isinstance(t, (tuple, list)) else nodes(t)
    assert route_ok(names, ran, not_ran), f"route not taken: wanted {ran} without {not_ran}, ran {sorted(names)}"
    return names


def producer(fn, k=0):
    """The class name of the node that feeds input k of the node fn."""
    return type(fn.next_functions[k][0]).__name__


@contextlib.contextmanager
def hooks(**kw):
    """Set the one-element test hooks of ops.core / ops.gpt2 for the block; restored after it."""
    from paddle_operator_amd.ops import core, gpt2
    cells = {k: getattr(core, k) if hasattr(core, k) else getattr(gpt2, k) for k in kw}
    saved = {k: c[0] for k, c in cells.items()}
    try:
        for k, v in kw.items():
            cells[k][0] = v
        yield
    finally:
        for k, c in cells.items():
            c[0] = saved[k]


@contextlib.contextmanager
def calls(m, *names):
    """Count the calls of the extension's functions `names` made by the ops inside the block (the ops
    look them up on the module at each call): which GEMM path a hook selected is not visible in the
    node classes, so the cases that force a library path assert these counts."""
    count = {n: 0 for n in names}
    real = {n: getattr(m, n) for n in names}

    def wrap(n):
        def f(*a, **kw):
            count[n] += 1
            return real[n](*a, **kw)
        return f

    try:
        for n in names:
            setattr(m, n, wrap(n))
        yield count
    finally:
        for n in names:
            setattr(m, n, real[n])


# ---------------------------------------------------------------------------------------------
# builders and references (CPU, float64; validated by test_gpt2_nodes_cpu.py)
# ---------------------------------------------------------------------------------------------
def grid(T, N, K):
    """The dyadic case of test_gemm_nt_exact_gpu.py for a [T, K] x [N, K]^T product (cached, shared)."""
    return ng.case(T, N, K, S_OF_K[K])


def gints(shape, seed, amax=G_MAX):
    return ng.ints(shape, amax, seed)


def grad_ints(T, N, seed):
    """The integer gradient [T, N] whose dW must be exact.  Up to T = 256 gemm_dw runs one split and
    the gradient is dense in [-15, 15].  Beyond it gemm_dw splits the token axis and rounds each
    split's partial to bf16 (test_gemm_dw_exact_gpu.py: part of the design), so every column holds
    SPARSE_NNZ entries of +-1: any partial sum over any token subset is at most 16 * 15 = 240 <= 256
    in magnitude, bf16-exact, and dW = RNE(base + exact) at every split count.  Every row still holds
    entries (asserted), so a dropped token row changes dW."""
    if T <= 256:
        return gints((T, N), seed)
    g = torch.Generator().manual_seed(seed)
    n, i = torch.arange(N).view(1, N), torch.arange(SPARSE_NNZ).view(-1, 1)
    assert T % (3 * SPARSE_NNZ) == 0 and N >= 48
    # column n: rows 3 n + (n // 16) % 3 + i T / 16 (mod T): distinct per column, and together every row
    rows = (3 * n + (n // 16) % 3 + i * (T // SPARSE_NNZ)) % T
    dy = torch.zeros(T, N, dtype=F64)
    dy.scatter_(0, rows, (2 * torch.randint(0, 2, rows.shape, generator=g) - 1).to(F64))
    assert SPARSE_NNZ * A_MAX <= 256 and bool((dy != 0).any(1).all())
    return dy


def either(got, wants, what):
    """got equals one of the expected bf16 tensors per element (library epilogues: one or two roundings)."""
    got = got.cpu()
    ok = torch.zeros(got.shape, dtype=torch.bool)
    for w in wants:
        ok |= got.view(torch.int16) == w.view(torch.int16)
    check_bits(got, torch.where(ok, got, wants[0]), what)


def linear_expect(c, dy, a=None, prev=None):
    """_LinearFn (or _LinearResFn) backward on the grid: dy [T, N] integers, a [T, K] integers (default
    the case's), prev = the arena's previous dW / db values (float64) or None.  Returns float64
    values: dx in units of 2^-s, dw and db integers; `two` holds the two-rounding forms of dw / db that
    a library accumulate may give."""
    a = c["a"] if a is None else a
    T, N, K = c["M"], c["N"], c["K"]
    assert N * G_MAX * B_MAG[1] < LIM, "dX sums are not exact"
    assert T * G_MAX * A_MAX + 2 * T * G_MAX * A_MAX < LIM, "dW sums onto a base are not exact"
    assert float(dy.abs().max()) <= G_MAX and float(a.abs().max()) <= A_MAX
    pw = dict(w=0.0, b=0.0) if prev is None else prev
    dw, db = dy.t() @ a, dy.sum(0)
    return dict(dx=rne(dy @ c["b"] + 0.0), dw=rne(pw["w"] + dw), db=rne(pw["b"] + db),
                two=dict(dw=rne(pw["w"] + rne(dw)), db=rne(pw["b"] + rne(db))))


def forward_expect(c):
    """y and the two residual forms h of the grid case, units of 2^-s: EPI 1, EPI 5 (one rounding) and
    GEMM + add_layernorm (two: r = RNE(P), then the fp32 sum (x + r) + b rounded)."""
    p, b, x = c["p"], c["bias"], ng.addend(c)
    return dict(y=rne(p + b), y_two=rne(rne(p) + b), plain=rne(p), h_fused=rne(p + b + x), h_unfused=rne(x + rne(p) + b))


def ln_case_of(v32, w, b):
    """The case dict check_ln_forward reads, for the fp32 rows v32 the LayerNorm kernel normalises."""
    c = dict(N=v32.shape[0], C=v32.shape[1], adv=False, v32=v32)
    c.update(ln_reference(v32.to(F64), w, b))
    return c


def stored_band(v):
    """|stored - v| for a bf16 activation output under check_activation's rule: the band plus half the
    bf16 spacing at the band's far edge."""
    band = DELTA * v.abs().clamp_min(BAND_FLOOR)
    return band + 0.5 * _quantum(v.abs() + band)


def behind(a, band_a, b, k_terms, split=False):
    """(ref, band) of a @ b where a is known within band_a per element and the GEMM adds k_terms fp32
    terms: sum |band| |b| + K 2^-24 sum |a b| (first order, times HO).  split: a gemm_dw that splits the
    token axis rounds each split's partial to bf16 before the fp32 fold: 2^-8 sum |a b| more (half a
    bf16 spacing is at most 2^-8 of the value)."""
    ref = a @ b
    band = (k_terms * U * HO + (2.0 ** -8 if split else 0.0)) * (a.abs() @ b.abs())
    if band_a is not None:
        band = band + band_a @ b.abs() + k_terms * U * (band_a @ b.abs())
    return ref, band


def accum_ok(first, second, alone=None):
    """Accumulation of an inexact gradient.  Every arena kernel forms the fp32 sum s and stores
    RNE(base + s).  `first` is the arena after one backward into zeros; `alone` = RNE(s2) is what the
    second micro-batch's backward gives on its own (default: the same inputs again, alone = first), so
    s2 lies within half a bf16 spacing q / 2 of it; after that second backward the arena holds
    RNE(first + s2), which must lie between RNE(first + alone - q / 2) and RNE(first + alone + q / 2).
    An accumulate flag clear on the second backward leaves `alone`, one set on the first after
    zero_grad() or a base added twice gives another sum: all outside (unless the elements are zero)."""
    f, g = first.double(), second.double()
    a = f if alone is None else alone.double()
    half = 0.5 * _quantum(a)
    return (g >= rne(f + a - half)) & (g <= rne(f + a + half))


def keep_mask(shape, spec):
    from paddle_operator_amd.ops import philox_keep_mask
    return philox_keep_mask(shape, spec.thr, spec.seed, spec.site, spec.step).to(F64)


def half_spec(site=3):
    """p = 0.5: thr = 32768 and the fp32 scale is exactly 2."""
    spec = _ops().dropout_spec(0.5, 0x1234567887654321, site, 7)
    assert spec.thr == 32768 and spec.scale == 2.0
    return spec


@functools.lru_cache(maxsize=None)
def lm_case():
    """The LM head on the grid: h [N, C] integers, W [Vp, C] on 2^-11, targets with -100, V, Vp - 1 and
    -1 among valid ones, every ignored target in the first chunk of 256 and one more in the second."""
    c = grid(LM_N, VP, C)
    g = torch.Generator().manual_seed(41)
    tgt = torch.randint(0, V, (LM_N,), generator=g)
    tgt[[3, 77, 130, 255]] = torch.tensor([-100, V, VP - 1, -1])
    tgt[300] = -100
    tgt[[0, 511]] = torch.tensor([0, V - 1])
    logits = as_bf16(rne(c["p"]) * c["u"])
    return dict(c=c, tgt=tgt, logits=logits, dead=~((tgt >= 0) & (tgt < V)))


def lm_reference(dloss=1.0, chunks=1, split=False):
    """float64 loss, dh and dW of the LM head with their propagated bands (module docstring); split:
    the dW GEMM of a chunk splits the token axis (behind())."""
    k = lm_case()
    c, tgt = k["c"], k["tgt"]
    loss, _, d, cnt = xent_ref(k["logits"], tgt, V, dloss)
    assert cnt == LM_N - 5
    band_d = XENT_REL * d.abs() + XENT_ABS * dloss / cnt
    band_d[k["dead"]] = 0.0
    band_d[:, V:] = 0.0
    w, h = c["b"] * c["u"], c["a"]
    dh, band_h = behind(d, band_d, w, VP)
    dw, band_w = behind(d.t(), band_d.t(), h, LM_N, split)
    band_w = band_w + (chunks - 1) * 2.0 ** -8 * (d.abs().t() @ h.abs())
    return dict(loss=loss, cnt=cnt, dh=dh, band_h=band_h, dw=dw, band_w=band_w)


# ---------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------
def dev(t, scale=1.0):
    return as_bf16(t * scale).cuda()


def leaf(t, scale=1.0):
    return dev(t, scale).requires_grad_()


class Params(torch.nn.Module):
    def __init__(self, **tensors):
        super().__init__()
        for n, t in tensors.items():
            setattr(self, n, torch.nn.Parameter(as_bf16(t).cuda()))


class Arena:
    """Parameters in a bf16 FlatParams arena (gradients written straight into it), with a count of the
    ready signals per parameter."""

    def __init__(self, split=(), late=(), **tensors):
        from paddle_operator_amd.parallel.flat import FlatParams
        self.mod = Params(**tensors)
        self.flat = FlatParams(self.mod, device="cuda", split=split, late=late)
        self.ready = {n: 0 for n in tensors}
        for n, p in self.mod.named_parameters():
            p._pdo_ready = functools.partial(self._count, n)

    def _count(self, n, p):
        self.ready[n] += 1

    def __getattr__(self, n):
        return getattr(self.__dict__["mod"], n)

    def grad(self, n):
        torch.cuda.synchronize()
        return getattr(self.mod, n).grad.detach().cpu().clone()


def grad2(t):
    return t.detach().cpu().reshape(-1, t.shape[-1])


def row(t):
    return t.detach().cpu().reshape(1, -1)


# ---------------------------------------------------------------------------------------------
# 1. _LinearFn
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (256, 768))
def test_linear_node_exact(cuda, T):
    """y, dX, dW and db of _LinearFn to the bit, as returned tensors and into the arena; a second
    backward with other inputs accumulates RNE(RNE(first) + second); zero_grad() gives the second alone."""
    ops, c = _ops(), grid(T, C, C)
    u, fw = c["u"], forward_expect(c)
    dy1, dy2, a2 = grad_ints(T, C, 11 + T), grad_ints(T, C, 12 + T), gints((T, C), 13 + T, A_MAX)
    assert T > 256 or _m().gemm_dw_splits(T, C, C) == 1
    e1 = linear_expect(c, dy1)
    a, w, b = leaf(c["a"]), leaf(c["b"], u), leaf(c["bias"], u)
    y = ops.linear(a, w, b)
    assert nodes(y) >= {"_LinearFnBackward"} and type(y.grad_fn).__name__ == "_LinearFnBackward"
    check_bits(y, as_bf16(fw["y"] * u), f"linear {T} y")
    y.backward(dev(dy1))
    check_bits(a.grad, as_bf16(e1["dx"] * u), f"linear {T} dX")
    check_bits(w.grad, as_bf16(e1["dw"]), f"linear {T} dW (returned)")
    check_bits(row(b.grad), as_bf16(e1["db"]).view(1, -1), f"linear {T} db (returned)")
    ar = Arena(w=c["b"] * u, b=c["bias"] * u)
    a = leaf(c["a"])
    ops.linear(a, ar.w, ar.b).backward(dev(dy1))
    check_bits(a.grad, as_bf16(e1["dx"] * u), f"linear {T} dX (arena)")
    check_bits(ar.grad("w"), as_bf16(e1["dw"]), f"linear {T} dW (arena)")
    check_bits(row(ar.grad("b")), as_bf16(e1["db"]).view(1, -1), f"linear {T} db (arena)")
    e2 = linear_expect(c, dy2, a2, prev=dict(w=e1["dw"], b=e1["db"]))
    ops.linear(dev(a2), ar.w, ar.b).backward(dev(dy2))
    check_bits(ar.grad("w"), as_bf16(e2["dw"]), f"linear {T} dW accumulated")
    check_bits(row(ar.grad("b")), as_bf16(e2["db"]).view(1, -1), f"linear {T} db accumulated")
    ar.flat.zero_grad()
    e3 = linear_expect(c, dy2, a2)
    ops.linear(dev(a2), ar.w, ar.b).backward(dev(dy2))
    check_bits(ar.grad("w"), as_bf16(e3["dw"]), f"linear {T} dW after zero_grad")
    check_bits(row(ar.grad("b")), as_bf16(e3["db"]).view(1, -1), f"linear {T} db after zero_grad")
    assert ar.ready == dict(w=3, b=3)


# name, T, K, hooks, and the calls of (gemm_nt, gemm_dw, transpose) that two forwards and two backwards
# make (the second input needs no gradient: one dX): the path a hook selects is not visible in the node class
LIB_ROUTES = [
    ("default", 256, 256, {}, (3, 2, 1)),
    ("ring", 256, 128, {}, (3, 2, 1)),                      # gemm_dw is asked and declines N = 128
    ("rows", 192, 256, {}, (0, 2, 1)),                      # M % 256 != 0: no gemm_nt, forward or dX
    ("nt_all", 256, 256, dict(_NT_ALL=0), (0, 2, 1)),
    ("dx_tn", 256, 256, dict(_DX_TN=False), (2, 2, 0)),     # dX = dy @ W: no W^T, no gemm_nt
    ("hip_dw", 256, 256, dict(_HIP_DW=False), (3, 0, 1)),
]


@pytest.mark.parametrize("name,T,K,hk,counts", LIB_ROUTES, ids=[r[0] for r in LIB_ROUTES])
def test_linear_fallback_routes_exact(cuda, name, T, K, hk, counts):
    """The ring (K = 128), the library (T = 192: M % 256 != 0) and each hook's library GEMM: the same
    exact products; a bias or an accumulate base may be rounded in once or after the product.  The
    extension calls made show that each hook and shape selected the path it names."""
    ops, m = _ops(), _m()
    c = ng.build_case(T, C, K, S_OF_K[K])
    u, fw = c["u"], forward_expect(c)
    assert bool(m.gemm_nt_supported(T, C, K)) == (name != "rows")
    assert bool(m.gemm_nt_epi_ok(T, C, K)) == (name not in ("rows", "ring"))
    dy1, dy2 = gints((T, C), 21 + T + K), gints((T, C), 22 + T + K)
    e1 = linear_expect(c, dy1)
    e2 = linear_expect(c, dy2, prev=dict(w=e1["dw"], b=e1["db"]))
    with hooks(**hk), calls(m, "gemm_nt", "gemm_dw", "transpose") as n:
        ar = Arena(w=c["b"] * u, b=c["bias"] * u)
        a = leaf(c["a"])
        y = ops.linear(a, ar.w, ar.b)
        assert type(y.grad_fn).__name__ == "_LinearFnBackward"
        either(y, [as_bf16(fw["y"] * u), as_bf16(fw["y_two"] * u)], f"linear {name} y")
        y.backward(dev(dy1))
        check_bits(a.grad, as_bf16(e1["dx"] * u), f"linear {name} dX")
        check_bits(ar.grad("w"), as_bf16(e1["dw"]), f"linear {name} dW")
        check_bits(row(ar.grad("b")), as_bf16(e1["db"]).view(1, -1), f"linear {name} db")
        ops.linear(dev(c["a"]), ar.w, ar.b).backward(dev(dy2))
        either(ar.grad("w"), [as_bf16(e2["dw"]), as_bf16(e2["two"]["dw"])], f"linear {name} dW accumulated")
        check_bits(row(ar.grad("b")), as_bf16(e2["db"]).view(1, -1), f"linear {name} db accumulated")
        assert ar.ready == dict(w=2, b=2)
    assert (n["gemm_nt"], n["gemm_dw"], n["transpose"]) == counts, (name, n)


@pytest.mark.parametrize("view", ("transposed", "sliced"))
def test_linear_noncontiguous_input_exact(cuda, view):
    """A transposed view and a sliced view of x: _LinearFn falls to routes that give the same exact
    y, dX and dW (the bias may be rounded in once or twice on the library)."""
    ops, T = _ops(), 256
    c = grid(T, C, C)
    u, fw = c["u"], forward_expect(c)
    dy = gints((T, C), 31)
    e = linear_expect(c, dy)
    if view == "transposed":
        base = dev(c["a"].t().contiguous()).requires_grad_()
        x = base.t()
    else:
        base = dev(torch.cat([c["a"], c["a"] + 1.0], 1)).requires_grad_()
        x = base[:, :C]
    assert not x.is_contiguous()
    ar = Arena(w=c["b"] * u, b=c["bias"] * u)
    y = ops.linear(x, ar.w, ar.b)
    assert type(y.grad_fn).__name__ == "_LinearFnBackward"
    either(y, [as_bf16(fw["y"] * u), as_bf16(fw["y_two"] * u)], f"linear {view} y")
    y.backward(dev(dy))
    dx = base.grad.t() if view == "transposed" else base.grad[:, :C]
    check_bits(dx.contiguous(), as_bf16(e["dx"] * u), f"linear {view} dX")
    check_bits(ar.grad("w"), as_bf16(e["dw"]), f"linear {view} dW")
    check_bits(row(ar.grad("b")), as_bf16(e["db"]).view(1, -1), f"linear {view} db")


def test_grouped_weight_gradients_exact(cuda):
    """deferred_weight_grads with _DW_CUS = 1: the queued dW GEMMs of two linears (1 + 4 tiles) run
    grouped (both in one launch when the 1-tile weight is queued first; when the 4-tile weight comes
    first it fills whole rounds and is flushed alone, the other at the scope's exit); with _DW_GROUPED
    off each runs on its own gemm_dw.  Both leave RNE(base + exact) in the
    arena over two backwards; n_grouped moves or does not; nothing is left queued."""
    from paddle_operator_amd.ops import core
    ops, m, T = _ops(), _m(), 256
    c1, c2 = grid(T, C, C), grid(T, HID, C)
    assert m.gemm_dw_grouped_ok(T, C, C) and m.gemm_dw_grouped_ok(T, HID, C)
    dys = {n: [gints((T, c["N"]), s), gints((T, c["N"]), s + 1)] for n, c, s in (("w1", c1, 51), ("w2", c2, 53))}
    want = {}
    for n, c in (("w1", c1), ("w2", c2)):
        e1 = linear_expect(c, dys[n][0])
        want[n] = [e1["dw"], linear_expect(c, dys[n][1], prev=dict(w=e1["dw"], b=0.0))["dw"]]
    for grouped in (True, False):
        with hooks(_DW_GROUPED=grouped, _DW_CUS=1):
            ar = Arena(w1=c1["b"] * c1["u"], w2=c2["b"] * c2["u"])
            n0 = core._dw_queue.n_grouped
            for k in range(2):
                y1, y2 = ops.linear(dev(c1["a"]), ar.w1), ops.linear(dev(c2["a"]), ar.w2)
                assert_route((y1, y2), ["_LinearFn"])
                with ops.deferred_weight_grads("cuda"):
                    torch.autograd.backward([y1, y2], [dev(dys["w1"][k]), dev(dys["w2"][k])])
                assert core._dw_queue.depth == 0 and not core._dw_queue.entries and core._dw_queue.held == 0
                for n in ("w1", "w2"):
                    check_bits(ar.grad(n), as_bf16(want[n][k]), f"dW {n} grouped={grouped} backward {k}")
            assert core._dw_queue.n_grouped - n0 == (4 if grouped else 0)
            assert ar.ready == dict(w1=2, w2=2)


# ---------------------------------------------------------------------------------------------
# 2. the residual nodes: _LinearResFn -> _LNResFn, _LinearFn -> _AddLayerNormFn, the Drop variants
# ---------------------------------------------------------------------------------------------
RES_ROUTES = {
    "fused": (dict(), 256, ["_LinearResFn", "_LNResFn"], ["_AddLayerNormFn", "_LinearFn"]),
    "fused768": (dict(), 768, ["_LinearResFn", "_LNResFn"], ["_AddLayerNormFn", "_LinearFn"]),
    "unfused": (dict(_RES_EPI=False), 256, ["_LinearFn", "_AddLayerNormFn"], ["_LinearResFn", "_LNResFn"]),
    "unfused768": (dict(_RES_EPI=False), 768, ["_LinearFn", "_AddLayerNormFn"], ["_LinearResFn", "_LNResFn"]),
    "rows192": (dict(), 192, ["_LinearFn", "_AddLayerNormFn"], ["_LinearResFn", "_LNResFn"]),
    # K = 128 < 256: _res_epi_ok keeps EPI 5 off the ring kernel
    "k128": (dict(), 256, ["_LinearFn", "_AddLayerNormFn"], ["_LinearResFn", "_LNResFn"]),
}
RES_K = {"k128": 128}    # the projection's input width where it is not C


def run_residual(ops, c, lnw, lnb, g1, g2, arena, P=None, a=None):
    """linear_add_layer_norm on the grid case (a: other integer activations; P: the parameters of an
    earlier call, to accumulate into); returns the outputs, the LayerNorm node's saved statistics and
    every gradient (CPU)."""
    u = c["u"]
    a, x = leaf(c["a"] if a is None else a), leaf(ng.addend(c), u)
    vals = dict(w=c["b"] * u, b=c["bias"] * u, lnw=lnw, lnb=lnb)
    if P is None:
        P = Arena(**vals) if arena else Params(**vals)
    h, y = ops.linear_add_layer_norm(a, P.w, P.b, x, P.lnw, P.lnb)
    names = nodes(h, y)
    saved = y.grad_fn.saved_tensors
    out = dict(names=names, h=h.detach().cpu(), y=y.detach().cpu(), mean=saved[2].cpu(), rstd=saved[3].cpu(),
               h_saved=saved[0].cpu(), top=type(y.grad_fn).__name__)
    # the node that feeds the LayerNorm: input 0 (h) of _LNResFn, input 1 (r) of _AddLayerNormFn
    out["feeds"] = producer(y.grad_fn, 0 if out["top"] == "_LNResFnBackward" else 1)
    torch.autograd.backward([h, y], [dev(g1), dev(g2)])
    torch.cuda.synchronize()
    out["grads"] = {n: (P.grad(n) if arena else getattr(P, n).grad.detach().cpu()) for n in vals}
    out["grads"].update(a=a.grad.cpu(), x=x.grad.cpu())
    out["ready"] = dict(P.ready) if arena else None
    out["P"] = P
    return out


@pytest.mark.parametrize("name", list(RES_ROUTES))
def test_residual_nodes_exact_chain(cuda, name):
    """h of each route to the bit (one rounding fused, two unfused).  LayerNorm weight zero: y = beta,
    dx = the downstream dh bit for bit, and the producer's da, dW, drbias = RNE(sum dh) and
    dbeta = RNE(sum dy) are exact, as returned tensors and in the arena; a second backward into the
    same arena with other activations and gradients leaves RNE(RNE(first) + second) in dW, drbias and
    dbeta."""
    hk, T, ran, not_ran = RES_ROUTES[name]
    ops, K = _ops(), RES_K.get(name, C)
    c = grid(T, C, K) if T != 192 else ng.build_case(T, C, K, S_OF_K[K])
    assert bool(_m().gemm_nt_epi_ok(T, C, K)) == (T != 192 and K >= 256)
    u, fw = c["u"], forward_expect(c)
    fused = "_LinearResFn" in ran
    g1, g2 = grad_ints(T, C, 61 + T), gints((T, C), 62 + T, 8)
    lnb = ng.GB_STEP * gints((C,), 63, 96)
    e = linear_expect(c, g1)
    h_want = as_bf16((fw["h_fused"] if fused else fw["h_unfused"]) * u)
    for arena in (False, True):
        with hooks(**hk):
            r = run_residual(ops, c, torch.zeros(C, dtype=F64), lnb, g1, g2, arena)
        assert route_ok(r["names"], ran, not_ran), (name, sorted(r["names"]))
        assert r["top"] == ("_LNResFnBackward" if fused else "_AddLayerNormFnBackward")
        assert r["feeds"] == ("_LinearResFnBackward" if fused else "_LinearFnBackward")
        what = f"residual {name} arena={arena}"
        check_bits(r["h"], h_want, f"{what} h")
        assert same_bits(r["h_saved"], h_want)
        assert bool((r["y"].double() == lnb).all()), f"{what}: y is not beta with a zero weight"
        G = r["grads"]
        check_bits(G["x"], as_bf16(g1), f"{what} dx = dh")
        check_bits(G["a"], as_bf16(e["dx"] * u), f"{what} da")
        check_bits(G["w"], as_bf16(e["dw"]), f"{what} dW")
        check_bits(row(G["b"]), as_bf16(e["db"]).view(1, -1), f"{what} drbias")
        check_bits(row(G["lnb"]), as_bf16(rne(g2.sum(0))).view(1, -1), f"{what} dbeta")
        if arena:
            assert r["ready"] == dict(w=1, b=1, lnw=1, lnb=1)
            a2, g1b, g2b = gints((T, K), 64 + T, A_MAX), grad_ints(T, C, 65 + T), gints((T, C), 66 + T, 8)
            e2 = linear_expect(c, g1b, a2, prev=dict(w=e["dw"], b=e["db"]))
            with hooks(**hk):
                r2 = run_residual(ops, c, None, None, g1b, g2b, True, P=r["P"], a=a2)
            assert route_ok(r2["names"], ran, not_ran)
            G2 = r2["grads"]
            check_bits(G2["x"], as_bf16(g1b), f"{what} dx = dh, second backward")
            either(G2["w"], [as_bf16(e2["dw"]), as_bf16(e2["two"]["dw"])] if K < 256 else [as_bf16(e2["dw"])],
                   f"{what} dW accumulated")     # K = 128: dW on the library's addmm_
            check_bits(row(G2["b"]), as_bf16(e2["db"]).view(1, -1), f"{what} drbias accumulated")
            check_bits(row(G2["lnb"]), as_bf16(rne(rne(g2.sum(0)) + g2b.sum(0))).view(1, -1), f"{what} dbeta accumulated")
            assert r2["ready"] == dict(w=2, b=2, lnw=2, lnb=2)


@pytest.mark.parametrize("name", ("fused", "fused768", "unfused", "unfused768"))
def test_residual_nodes_layernorm_bands(cuda, name):
    """Random LayerNorm weights and gradients on the exactly known h: mean, rstd and y by
    check_ln_forward; dx (read as x.grad), dgamma, dbeta and drbias by ln_bwd_reference from the node's
    own statistics; the arena route gives the returned route's bits."""
    hk, T, ran, not_ran = RES_ROUTES[name]
    ops, c = _ops(), grid(T, C, C)
    u, fw = c["u"], forward_expect(c)
    fused = "_LinearResFn" in ran
    gen = torch.Generator().manual_seed(71 + T)
    lnw, lnb, g1, g2 = (randn16(s, gen) for s in ((C,), (C,), (T, C), (T, C)))
    # the fp32 rows the LayerNorm kernel normalises: the stored bf16 h (fused), the exact fp32 sum (unfused)
    v = (fw["h_fused"] if fused else ng.addend(c) + fw["plain"] + c["bias"]) * u
    lc = ln_case_of(v.to(torch.float32), lnw, lnb)
    with hooks(**hk):
        r = run_residual(ops, c, lnw, lnb, g1, g2, False)
        ra = run_residual(ops, c, lnw, lnb, g1, g2, True)
    assert route_ok(r["names"], ran, not_ran) and route_ok(ra["names"], ran, not_ran)
    what = f"residual {name}"
    check_ln_forward(lc, r["mean"], r["rstd"], r["y"], r["h"], what)
    ref = ln_bwd_reference(r["h"].double(), g2, lnw, r["mean"].double(), r["rstd"].double(), g1)
    G = r["grads"]
    check_banded(G["x"], ref["dx"], ref["band"], f"{what} dx", wide_cap=WIDE_CAP)
    worst = {n: check_colgrad(n, G[p], ref, what) for n, p in (("dgamma", "lnw"), ("dbeta", "lnb"), ("drbias", "b"))}
    record(f"{what}: worst (|got - sum| - half a spacing) / bound: " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    for n in G:
        assert same_bits(ra["grads"][n], G[n]), f"{what}: arena gradient {n} differs from the returned one"
    assert same_bits(ra["y"], r["y"]) and same_bits(ra["h"], r["h"])


def test_dropout_residual_nodes_exact(cuda):
    """_AddLayerNormDropFn at p = 0.5 on the grid with a zero LayerNorm weight: h = RNE(x + 2 keep (r +
    rbias)), dx = dh unmasked, dr = 2 keep dh, drbias = RNE(sum 2 keep dh).  _LNResDropFn returns the
    masked de and no dx.  drop=None and thr == 0 reach the plain node classes."""
    ops, T = _ops(), 256
    c = grid(T, C, C)
    u = c["u"]
    spec = half_spec()
    keep = keep_mask((T, C), spec)
    assert 0.45 < float(keep.mean()) < 0.55
    x, rr, rb = ng.addend(c), 4.0 * gints((T, C), 81, 255), c["bias"]
    g1, g2 = gints((T, C), 82), gints((T, C), 83, 8)
    lnb = ng.GB_STEP * gints((C,), 84, 96)
    for arena in (False, True):
        vals = dict(lnw=torch.zeros(C, dtype=F64), lnb=lnb, rb=rb * u)
        P = Arena(**vals) if arena else Params(**vals)
        xl, rl = leaf(x, u), leaf(rr, u)
        h, y = ops.add_layer_norm(xl, rl, P.lnw, P.lnb, rbias=P.rb, drop=spec)
        assert_route((h, y), ["_AddLayerNormDropFn"], ["_AddLayerNormFn"])
        what = f"add_layer_norm drop arena={arena}"
        check_bits(h, as_bf16(rne(x + 2.0 * keep * (rr + rb)) * u), f"{what} h")
        torch.autograd.backward([h, y], [dev(g1), dev(g2)])
        check_bits(xl.grad, as_bf16(g1), f"{what} dx unmasked")
        want_dr = 2.0 * keep * g1
        assert bool((rl.grad.cpu().double() == want_dr).all()), f"{what}: dr is not 2 keep dh"
        assert bool(((rl.grad.cpu() != 0) <= (keep > 0)).all()), f"{what}: dr is non-zero where dropped"
        drb = P.grad("rb") if arena else P.rb.grad.cpu()
        check_bits(row(drb), as_bf16(rne(want_dr.sum(0))).view(1, -1), f"{what} drbias sums the masked gradient")
        dbeta = P.grad("lnb") if arena else P.lnb.grad.cpu()
        check_bits(row(dbeta), as_bf16(rne(g2.sum(0))).view(1, -1), f"{what} dbeta")
    # _LNResDropFn: the producer receives the masked, scaled gradient
    P = Params(lnw=torch.zeros(C, dtype=F64), lnb=lnb)
    for drop, node, want in ((spec, "_LNResDropFn", 2.0 * keep * g1), (None, "_LNResFn", g1),
                             (ops.Dropout(0, 1.0, 1, 2, 3), "_LNResFn", g1)):
        e = leaf(x, u)
        h, y = ops.layer_norm_res(e.clone(), P.lnw, P.lnb, drop=drop)
        names = assert_route((h, y), [node], ["_LNResDropFn"] if node == "_LNResFn" else ["_LNResFn"])
        assert "_LayerNormFnBackward" not in names
        torch.autograd.backward([h, y], [dev(g1), dev(g2)])
        assert bool((e.grad.cpu().double() == want).all()), f"layer_norm_res drop={drop}: wrong producer gradient"
    # drop=None and thr == 0 on add_layer_norm
    for drop in (None, ops.dropout_spec(0.0, 1, 2, 3), ops.Dropout(0, 1.0, 1, 2, 3)):
        h, y = ops.add_layer_norm(leaf(x, u), leaf(rr, u), P.lnw, P.lnb, rbias=None, drop=drop)
        assert_route((h, y), ["_AddLayerNormFn"], ["_AddLayerNormDropFn"])
        check_bits(h, as_bf16(rne(x + rr) * u), "add_layer_norm without dropout h")
    # a non-contiguous x: layer_norm_res falls to _LayerNormFn on a contiguous copy
    # (the same kernels on the same values): h, y and every gradient have the bits of the contiguous call
    gen = torch.Generator().manual_seed(85)
    lnw, gy, gh = randn16((C,), gen), randn16((T, C), gen), randn16((T, C), gen)
    outs = {}
    for kind in ("contiguous", "transposed", "sliced"):
        Q = Params(lnw=lnw, lnb=lnb)
        if kind == "contiguous":
            src = leaf(x, u)
            xin = src.clone()
        elif kind == "transposed":
            src = dev((x * u).t().contiguous()).requires_grad_()
            xin = src.t()
        else:
            src = dev(torch.cat([x * u, x * u], 1)).requires_grad_()
            xin = src[:, :C]
        assert xin.is_contiguous() == (kind == "contiguous")
        h, y = ops.layer_norm_res(xin, Q.lnw, Q.lnb)
        if kind == "contiguous":
            assert_route((h, y), ["_LNResFn"], ["_LayerNormFn"])
        else:
            assert_route(y, ["_LayerNormFn"], ["_LNResFn"])
        torch.autograd.backward([h, y], [dev(gh), dev(gy)])
        dx = src.grad if kind == "contiguous" else (src.grad.t() if kind == "transposed" else src.grad[:, :C])
        outs[kind] = dict(h=h.detach().cpu(), y=y.detach().cpu(), dx=dx.contiguous().cpu(),
                          dw=Q.lnw.grad.cpu(), db=Q.lnb.grad.cpu())
    for kind in ("transposed", "sliced"):
        for n, t in outs[kind].items():
            if n == "dx":
                # _LNResFn adds the residual gradient inside the kernel (one rounding); the view's route adds
                # it in autograd after the LayerNorm's dx was rounded: held to that two-rounding form below
                continue
            assert same_bits(t, outs["contiguous"][n]), f"layer_norm_res on a {kind} view: {n} differs"
    # dx of the view routes: RNE(RNE(LayerNorm dx) + dh), from the contiguous kernel run without dh
    Q = Params(lnw=lnw, lnb=lnb)
    xin = leaf(x, u)
    ops.layer_norm(xin, Q.lnw, Q.lnb).backward(dev(gy))
    want = (xin.grad.cpu().float() + as_bf16(gh).float()).to(BF16)
    for kind in ("transposed", "sliced"):
        check_bits(outs[kind]["dx"], want, f"layer_norm_res on a {kind} view: dx")


def test_linear_add_layer_norm_view_and_drop_routes(cuda):
    """A non-contiguous `a` takes _LinearFn -> _AddLayerNormFn with the two-rounding h; drop= takes
    _LinearFn -> _AddLayerNormDropFn with h = RNE(x + 2 keep (RNE(P) + b))."""
    ops, T = _ops(), 256
    c = grid(T, C, C)
    u, fw = c["u"], forward_expect(c)
    P = Params(w=c["b"] * u, b=c["bias"] * u, lnw=torch.ones(C, dtype=F64), lnb=torch.zeros(C, dtype=F64))
    a = dev(c["a"].t().contiguous()).t().requires_grad_()
    h, y = ops.linear_add_layer_norm(a, P.w, P.b, leaf(ng.addend(c), u), P.lnw, P.lnb)
    assert_route((h, y), ["_LinearFn", "_AddLayerNormFn"], ["_LinearResFn", "_LNResFn"])
    check_bits(h, as_bf16(fw["h_unfused"] * u), "linear_add_layer_norm transposed a: h")
    spec = half_spec(5)
    keep = keep_mask((T, C), spec)
    h, y = ops.linear_add_layer_norm(leaf(c["a"]), P.w, P.b, leaf(ng.addend(c), u), P.lnw, P.lnb, drop=spec)
    assert_route((h, y), ["_LinearFn", "_AddLayerNormDropFn"], ["_LinearResFn", "_LNResFn", "_AddLayerNormFn"])
    check_bits(h, as_bf16(rne(ng.addend(c) + 2.0 * keep * (fw["plain"] + c["bias"])) * u), "linear_add_layer_norm drop: h")


# ---------------------------------------------------------------------------------------------
# 3. the MLP nodes
# ---------------------------------------------------------------------------------------------
MLP_ROUTES = {
    "saved": (dict(), 256, ["_NTMLPFn"], ["_GeluLinearFn", "_BiasGeluFn", "_LinearFn"]),
    "saved768": (dict(), 768, ["_NTMLPFn"], ["_GeluLinearFn", "_BiasGeluFn", "_LinearFn"]),
    "recompute": (dict(_NT_GD=False), 256, ["_NTMLPFn"], ["_GeluLinearFn", "_BiasGeluFn", "_LinearFn"]),
    "gelu_linear": (dict(_NT_GELU=False), 256, ["_LinearFn", "_GeluLinearFn"], ["_NTMLPFn", "_BiasGeluFn"]),
    "bias_gelu": (dict(_NT_DGELU=False), 256, ["_LinearFn", "_BiasGeluFn"], ["_NTMLPFn", "_GeluLinearFn"]),
    "rows192": (dict(), 192, ["_LinearFn", "_BiasGeluFn"], ["_NTMLPFn", "_GeluLinearFn"]),
    # mlp_add_layer_norm without the residual epilogue: _NTMLPFn (no res) feeds _AddLayerNormFn
    "res_epi_off": (dict(_RES_EPI=False), 256, ["_NTMLPFn"], ["_GeluLinearFn", "_BiasGeluFn", "_LinearFn"]),
}


def mlp_cases(T):
    mk = grid if T % 256 == 0 else (lambda t, n, k: ng.build_case(t, n, k, S_OF_K[k]))
    return mk(T, HID, C), mk(T, C, HID)


def mlp_forward_reference(c1, fused):
    """(hp = RNE(P), float64 GELU argument, gelu, gelu') of fc1: the fused epilogue sees the fp32 P,
    the unfused kernel the stored bf16 RNE(P); the bias joins in fp32 (exact on the grid)."""
    pv = c1["p"] * c1["u"]
    hp = rne(pv)
    arg = (pv if fused else hp) + c1["gbias"]
    assert float(arg.abs().max()) <= ng.X_LIMIT
    return dict(hp=hp, arg=arg, h=lg.gelu_ref(arg), gd=lg.gelu_grad_ref(arg))


def mlp_backward_reference(route, c1, c2, h, saved, g, split=False):
    """float64 gradients of the MLP node from its stored h (bf16 values) and `saved` (the stored gelu'
    or pre-activation), for the integer gradient g [T, C] of its output.  Returns name -> (ref, band).
    split: the dW GEMMs split the token axis (behind())."""
    T = g.shape[0]
    u2 = c2["u"]
    w1, w2, x = c1["b"] * c1["u"], c2["b"] * u2, c1["a"]
    assert C * G_MAX * B_MAG[1] < LIM
    p2 = (g @ c2["b"] + 0.0) * u2                         # exact in the fp32 accumulators
    if route == "saved":                                  # EPI 8: one fp32 multiply, one bf16 rounding
        dhp = (p2 * saved).to(torch.float32).to(BF16).to(F64)
        band, d_unrounded = None, (p2 * saved)
    else:
        arg = lg.gelu_arg(saved, c1["gbias"])             # the fp32 sum pre + b1
        lhs = rne(p2) if route == "bias_gelu" else p2     # _BiasGeluFn reads the stored dh = RNE(P)
        dhp = lhs * gelu_grad64(arg)
        band, d_unrounded = stored_band(dhp), dhp
    out = dict(dw2=behind(g.t(), None, h, T, split), dx=behind(dhp, band, w1, HID),
               dw1=behind(dhp.t(), None if band is None else band.t(), x, T, split))
    s = d_unrounded.sum(0)
    out["db1"] = (s, db_bound(s, d_unrounded.abs().sum(0), T))
    return out


def run_mlp(ops, c1, c2, g, arena, res, hk):
    u1, u2 = c1["u"], c2["u"]
    vals = dict(w1=c1["b"] * u1, b1=c1["gbias"], w2=c2["b"] * u2)
    if res:
        vals.update(b2=c2["bias"] * u2, lnw=torch.zeros(C, dtype=F64), lnb=torch.ones(C, dtype=F64))
    P = Arena(**vals) if arena else Params(**vals)
    x = leaf(c1["a"])
    with hooks(**hk):
        if res:
            r = leaf(ng.addend(c2), u2)
            out, y = ops.mlp_add_layer_norm(x, P.w1, P.b1, P.w2, P.b2, r, P.lnw, P.lnb)
            # the MLP's last node feeds input 0 (h) of _LNResFn or input 1 (r) of _AddLayerNormFn
            k = 0 if type(y.grad_fn).__name__ == "_LNResFnBackward" else 1
            names, node = nodes(out, y), y.grad_fn.next_functions[k][0]
        else:
            out = ops.mlp(x, P.w1, P.b1, P.w2)
            names, node, r = nodes(out), out.grad_fn, None
        saved = [t.cpu() for t in node.saved_tensors]
        o = dict(names=names, out=out.detach().cpu(), saved=saved, node=type(node).__name__)
        if res:
            torch.autograd.backward([out, y], [dev(g), torch.zeros_like(y)])
        else:
            out.backward(dev(g))
        torch.cuda.synchronize()
    o["grads"] = {n: (P.grad(n) if arena else getattr(P, n).grad.detach().cpu()) for n in vals}
    o["grads"]["x"] = x.grad.cpu()
    if res:
        o["grads"]["res"] = r.grad.cpu()
    o["ready"] = P.ready if arena else None
    return o


@pytest.mark.parametrize("res", (False, True), ids=("mlp", "mlp_add_layer_norm"))
@pytest.mark.parametrize("name", list(MLP_ROUTES))
def test_mlp_nodes(cuda, name, res):
    """Every MLP route: the node classes; the stored pre-activation / gelu' and gelu output against the
    float64 GELU of the route's own argument; the output per element against the float64 product of
    the stored h (plus b2 and res, with one rounding behind the residual epilogue and two behind
    _AddLayerNormFn) and bit for bit against the same GEMM called on it; every gradient within its
    propagated band; with res, dres = the incoming gradient bit for bit and db2 = RNE(sum dy); the
    arena route gives the returned route's bits."""
    hk, T, ran, not_ran = MLP_ROUTES[name]
    ops, m = _ops(), _m()
    c1, c2 = mlp_cases(T)
    u2 = c2["u"]
    g = gints((T, C), 91 + T)
    ran, not_ran = list(ran), list(not_ran)
    res_epi = res and ran == ["_NTMLPFn"] and hk.get("_RES_EPI", True)   # fc2's epilogue adds b2 and res
    if res:
        ran += ["_LNResFn"] if res_epi else ["_AddLayerNormFn"]
        not_ran += ["_AddLayerNormFn"] if res_epi else ["_LNResFn"]
    r = run_mlp(ops, c1, c2, g, False, res, hk)
    ra = run_mlp(ops, c1, c2, g, True, res, hk)
    what = f"{'mlp_add_layer_norm' if res else 'mlp'} {name}"
    assert route_ok(r["names"], ran, not_ran) and route_ok(ra["names"], ran, not_ran), (what, sorted(r["names"]))
    fused = ran[0] == "_NTMLPFn"
    fr = mlp_forward_reference(c1, fused)
    if fused:
        assert r["node"] == "_NTMLPFnBackward"
        _, _, hp, h, _ = r["saved"]
        route = "saved" if "_NT_GD" not in hk else "recompute"
        if route == "saved":
            check_activation(hp, fr["gd"], f"{what} stored gelu'")
        else:
            check_bits(hp, as_bf16(fr["hp"]), f"{what} stored pre-activation")
        check_activation(h, fr["h"], f"{what} h")
    elif "_GeluLinearFn" in ran:
        route = "recompute"
        assert r["node"] == "_GeluLinearFnBackward"
        hp, h, _ = r["saved"]
        check_bits(hp, as_bf16(fr["hp"]), f"{what} hp of fc1")
        check_activation(h, fr["h"], f"{what} h")
    else:
        route = "bias_gelu"
        assert r["node"] == "_LinearFnBackward"
        h, hp = r["saved"][0], as_bf16(fr["hp"])       # fc2's _LinearFn saved (x = the gelu output, w)
        check_activation(h, fr["h"], f"{what} h")
    h64 = h.double()
    w2v = c2["b"] * u2
    ref, band = behind(h64, None, w2v.t(), HID)
    extra = c2["bias"] * u2 + ng.addend(c2) * u2
    if res_epi:                                          # bias and residual join the accumulator: one rounding
        ref, band = ref + extra, band + 2 * U * (ref.abs() + extra.abs())
        direct = m.gemm_nt_add(h.cuda(), dev(w2v), dev(ng.addend(c2), u2), bias=dev(c2["bias"], u2))
        assert same_bits(direct.cpu(), r["out"]), f"{what}: not the bits of gemm_nt_add on the stored h"
        check_banded(r["out"], ref, band, f"{what} out")
    elif not res:
        check_banded(r["out"], ref, band, f"{what} out")
        if T % 256 == 0:
            assert same_bits(m.gemm_nt(h.cuda(), dev(w2v)).cpu(), r["out"]), f"{what}: not gemm_nt on the stored h"
    else:
        # two roundings: the GEMM stores r = RNE(h W2^T), the add + LayerNorm kernel forms the fp32 sum
        # (res + r) + b2 and rounds it.  Per element: r within the GEMM band plus half its bf16 spacing,
        # two fp32 additions; a bias added twice (in an epilogue and as rbias) is outside.  Bit for bit:
        # that fp32 sum, formed on the host from the same GEMM called on the stored h.
        band = band + 0.5 * _quantum(ref.abs() + band) + 2 * U * (ref.abs() + extra.abs())
        check_banded(r["out"], ref + extra, band, f"{what} out")
        rr = (m.gemm_nt(h.cuda(), dev(w2v)) if T % 256 == 0 else torch.nn.functional.linear(h.cuda(), dev(w2v))).cpu()
        f32 = torch.float32
        want = ((as_bf16(ng.addend(c2) * u2).to(f32) + rr.to(f32)) + as_bf16(c2["bias"] * u2).to(f32)).to(BF16)
        check_bits(r["out"], want, f"{what} out = RNE((res + r) + b2)")
    split = m.gemm_dw_splits(T, HID, C) > 1 or m.gemm_dw_splits(T, C, HID) > 1
    refs = mlp_backward_reference(route, c1, c2, h64, hp.double(), g, split)
    G = r["grads"]
    got = dict(dw2=G["w2"], dw1=G["w1"], dx=G["x"])
    for n, t in got.items():
        check_banded(t.reshape(refs[n][0].shape), refs[n][0], refs[n][1], f"{what} {n}")
    s, bound = refs["db1"]
    ratio = (G["b1"].double() - s).abs() / bound
    record(f"{what} db1: worst |err| / bound {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0, f"{what} db1: column {int(ratio.argmax())} at {float(ratio.max()):.3f} of its bound"
    if res:
        check_bits(G["res"], as_bf16(g), f"{what} dres = dy")
        check_bits(row(G["b2"]), as_bf16(rne(g.sum(0))).view(1, -1), f"{what} db2")
    for n in G:
        assert same_bits(ra["grads"][n], G[n]), f"{what}: arena gradient {n} differs from the returned one"
    assert same_bits(ra["out"], r["out"])
    if ra["ready"] is not None:
        assert all(v == 1 for v in ra["ready"].values()), ra["ready"]


# ---------------------------------------------------------------------------------------------
# 4. attention
# ---------------------------------------------------------------------------------------------
def heads(t):
    return ax.to_heads(t, HEADS)


@pytest.mark.parametrize("S", (128, 384))
def test_qkv_attention_nodes(cuda, S):
    """_QKVAttnFn on the grid: the qkv it builds is RNE(P + b) to the bit and feeds attention's float64
    references (check_forward, check_backward); with _QKV_FUSED off the same kernels run as _LinearFn
    -> _FlashAttnFn: o, dh and dW are bit-identical, db lies inside check_db's interval of the observed
    dqkv, and the arena route gives the returned route's bits."""
    ops, B = _ops(), 2
    T = B * S
    c = grid(T, 3 * C, C)
    u = c["u"]
    qkv_want = as_bf16(forward_expect(c)["y"] * u)
    do = randn16((B, S, C), torch.Generator().manual_seed(101 + S))
    vals = dict(w=c["b"] * u, b=c["bias"] * u)
    runs = {}
    for mode in ("fused", "fused-arena", "unfused"):
        P = Arena(**vals) if mode == "fused-arena" else Params(**vals)
        hx = leaf(c["a"].reshape(B, S, C))
        with hooks(_QKV_FUSED=mode != "unfused"):
            if mode == "unfused":
                assert_route(ops.qkv_attention(hx, P.w, P.b, HEADS), ["_LinearFn", "_FlashAttnFn"], ["_QKVAttnFn"])
                qkv = ops.linear(hx, P.w, P.b)
                qkv.retain_grad()
                o = ops.attention(qkv, HEADS)
                assert_route(o, ["_LinearFn", "_FlashAttnFn"], ["_QKVAttnFn"])
                saved_qkv, _, lse = o.grad_fn.saved_tensors
            else:
                o = ops.qkv_attention(hx, P.w, P.b, HEADS)
                assert_route(o, ["_QKVAttnFn"], ["_LinearFn", "_FlashAttnFn"])
                _, _, saved_qkv, _, lse = o.grad_fn.saved_tensors
            check_bits(grad2(saved_qkv), qkv_want, f"qkv_attention {mode} S={S}: the qkv fed to attention")
            lse = lse.clone()
            o.backward(dev(do))
        torch.cuda.synchronize()
        grads = {n: (P.grad(n) if mode == "fused-arena" else getattr(P, n).grad.detach().cpu()) for n in vals}
        runs[mode] = dict(o=o.detach(), lse=lse, dh=hx.grad.cpu(), grads=grads,
                          dqkv=qkv.grad.detach() if mode == "unfused" else None)
    q, k, v = (t.double() for t in ax.split_dqkv(qkv_want.cuda().reshape(B, S, 3 * C), HEADS))
    what = f"qkv_attention S={S}"
    f = runs["fused"]
    ax.check_forward(ax.forward_reference(q, k, v), heads(f["o"]), f["lse"], what)
    un = runs["unfused"]
    dq, dk, dv = ax.split_dqkv(un["dqkv"], HEADS)
    ref = ax.backward_reference(q, k, v, heads(dev(do)).double(), heads(un["o"]).double(), un["lse"].double())
    ax.check_backward(ref, dq, dk, dv, what)
    rdb = ax.check_db(f["grads"]["b"].cuda(), un["dqkv"], f"{what} fused db")
    record(f"{what}: fused db beyond rounding / bound {rdb:.3f}")
    for mode in ("fused-arena", "unfused"):
        r = runs[mode]
        assert same_bits(r["o"], f["o"]) and same_bits(r["lse"], f["lse"]), f"{what}: {mode} o / lse differ"
        assert same_bits(r["dh"], f["dh"]), f"{what}: {mode} dh differs from the fused node's"
        assert same_bits(r["grads"]["w"], f["grads"]["w"]), f"{what}: {mode} dW differs from the fused node's"
    assert same_bits(runs["fused-arena"]["grads"]["b"], f["grads"]["b"]), f"{what}: arena db differs"
    ax.check_db(un["grads"]["b"].cuda(), un["dqkv"], f"{what} unfused db")
    # dW and dh of the fused node against the exact chain cannot be stated (dqkv is not on a grid);
    # the unfused route's dW is gemm_dw of the observed dqkv, per element within T fp32 additions
    refw, bandw = behind(un["dqkv"].cpu().double().reshape(T, 3 * C).t(), None, c["a"], T,
                         _m().gemm_dw_splits(T, 3 * C, C) > 1)
    check_banded(f["grads"]["w"], refw, bandw, f"{what} dW")
    refh, bandh = behind(un["dqkv"].cpu().double().reshape(T, 3 * C), None, c["b"] * u, 3 * C)
    check_banded(f["dh"].reshape(T, C), refh, bandh, f"{what} dh")


@pytest.mark.parametrize("n_head,S,why", [(8, 128, "head dim 32"), (4, 96, "S % 128 != 0")])
def test_attention_fallback_routes(cuda, n_head, S, why):
    """Shapes outside the flash kernels' contract take _LinearFn and the framework attention: no
    flash node runs, and the output is finite."""
    ops, B = _ops(), 2
    gen = torch.Generator().manual_seed(S + n_head)
    hx = dev(randn16((B, S, C), gen)).requires_grad_()
    w, b = leaf(randn16((3 * C, C), gen, 0.05)), leaf(randn16((3 * C,), gen, 0.1))
    o = ops.qkv_attention(hx, w, b, n_head)
    names = assert_route(o, ["_LinearFn"], ["_QKVAttnFn", "_FlashAttnFn"])
    assert any("ScaledDotProduct" in n or "Attention" in n for n in names), (why, sorted(names))
    o.float().sum().backward()
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(hx.grad.float()).all())


# ---------------------------------------------------------------------------------------------
# 5. the LM head
# ---------------------------------------------------------------------------------------------
def run_lm(ops, hk, dloss=1.0, w=None):
    k = lm_case()
    c = k["c"]
    h = leaf(c["a"])
    w = leaf(c["b"], c["u"]) if w is None else w
    with hooks(**hk):
        loss = ops.lm_head_xent(h, w, k["tgt"].cuda(), V)
        names = nodes(loss)
        loss.backward(torch.tensor(dloss, device="cuda"))
    torch.cuda.synchronize()
    return dict(loss=float(loss.detach()), names=names, dh=h.grad.cpu(), dw=None if w.grad is None else w.grad.detach().cpu())


def lm_split(chunks):
    return _m().gemm_dw_splits(LM_N // chunks, VP, C) > 1


def check_lm(r, ref, what):
    k = lm_case()
    tol = LOSS_REL * max(1.0, ref["loss"]) + LM_N * U * ref["loss"]
    record(f"{what}: loss {r['loss']:.6f}, float64 {ref['loss']:.6f} (count {ref['cnt']})")
    assert abs(r["loss"] - ref["loss"]) <= tol, f"{what}: loss {r['loss']!r} against {ref['loss']!r}"
    assert bool((r["dh"][k["dead"]] == 0).all()), f"{what}: a token with an ignored target has a gradient"
    assert bool((r["dw"][V:] == 0).all()), f"{what}: a padding row of dW is non-zero"
    assert bool((r["dh"][~k["dead"]] != 0).any(1).all()), f"{what}: a valid token has no gradient"
    check_banded(r["dh"], ref["dh"], ref["band_h"], f"{what} dh")
    check_banded(r["dw"], ref["dw"], ref["band_w"], f"{what} dW")


LM_ROUTES = [
    ("whole", dict(_LM_CHUNK=-1), 1, ["_LMHeadXentFn"], ["_XentFn", "_LinearFn"]),
    ("chunk256", dict(_LM_CHUNK=256), 2, ["_LMHeadXentFn"], ["_XentFn", "_LinearFn"]),
    ("two-kernel", dict(_LM_CHUNK=256, _XENT_FUSED=False), 2, ["_LMHeadXentFn"], ["_XentFn", "_LinearFn"]),
    ("separate", dict(_LM_CHUNK=0), 1, ["_LinearFn", "_XentFn"], ["_LMHeadXentFn"]),
]


@pytest.mark.parametrize("name,hk,chunks,ran,not_ran", LM_ROUTES, ids=[r[0] for r in LM_ROUTES])
def test_lm_head_routes(cuda, name, hk, chunks, ran, not_ran):
    """Ignored targets (-100, V, Vp - 1, -1) get zero dh rows, dW[V:Vp] is zero, the loss is the mean
    over the valid rows of all chunks, dh and dW lie within the bands propagated from the dlogits rule."""
    r = run_lm(_ops(), hk)
    assert route_ok(r["names"], ran, not_ran), (name, sorted(r["names"]))
    check_lm(r, lm_reference(1.0, chunks, lm_split(chunks)), f"lm_head {name}")


def test_lm_head_dloss_chunks_and_no_grad(cuda):
    """backward(0.5) is exactly half of backward(1), bit for bit (scale_dev_: one rounding, and a
    halving is exact); chunk 256 gives chunk -1's dh bit for bit and a dW within the chunked band; the
    no_grad route returns the same loss within the same bound."""
    ops = _ops()
    one, half = run_lm(ops, dict(_LM_CHUNK=-1)), run_lm(ops, dict(_LM_CHUNK=-1), 0.5)
    for n in ("dh", "dw"):
        assert same_bits(half[n], as_bf16(one[n].double() * 0.5)), f"lm_head: {n} at dloss 0.5 is not half of dloss 1"
    check_lm(half, lm_reference(0.5, 1, lm_split(1)), "lm_head dloss 0.5")
    ch = run_lm(ops, dict(_LM_CHUNK=256))
    assert same_bits(ch["dh"], one["dh"]), "lm_head: chunk 256 and chunk -1 give different dh bits"
    record(f"lm_head: dW of chunk 256 differs from chunk -1 in {int((ch['dw'] != one['dw']).sum())} of {ch['dw'].numel()}")
    k = lm_case()
    ref = lm_reference()
    hd, wd, td = dev(k["c"]["a"]), dev(k["c"]["b"], k["c"]["u"]), k["tgt"].cuda()
    for chunk in (-1, 256):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with hooks(_LM_CHUNK=chunk), torch.no_grad():
            loss = ops.lm_head_xent(hd, wd, td, V)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        assert loss.grad_fn is None
        assert abs(float(loss) - ref["loss"]) <= LOSS_REL * max(1.0, ref["loss"]) + LM_N * U * ref["loss"]
        # beside the [chunk, Vp] logits there is no room for a [Vp, C] buffer (dW, or a W^T copy)
        rows = LM_N if chunk < 0 else chunk
        record(f"lm_head no_grad chunk {chunk}: peak allocation {peak} bytes, logits {rows * VP * 2}")
        assert peak < rows * VP * 2 + VP * C * 2, f"lm_head no_grad chunk {chunk}: {peak} bytes allocated"


def test_lm_head_against_the_observed_dlogits(cuda):
    """linear + cross_entropy called apart make dlogits observable (logits.grad, written in place): it
    obeys the cross-entropy rule with zero rows for ignored targets and zero padding columns; dh and dW
    are then the float64 products of that stored dlogits within the GEMMs' own K 2^-24 sum |terms|.
    _LMHeadXentFn with xent_fwd + xent_bwd over one chunk runs the same kernels on the same bits: its
    dh and dW are identical."""
    from test_small_kernels_gpu import _check_dlogits
    ops, m, k = _ops(), _m(), lm_case()
    c = k["c"]
    h, w = leaf(c["a"]), leaf(c["b"], c["u"])
    logits = ops.linear(h, w)
    check_bits(logits, k["logits"], "the LM head's logits")
    logits.retain_grad()
    loss = ops.cross_entropy(logits, k["tgt"].cuda(), V)
    assert_route(loss, ["_LinearFn", "_XentFn"], ["_LMHeadXentFn"])
    loss.backward()
    torch.cuda.synchronize()
    dl = logits.grad.detach().cpu()
    _, _, d, cnt = xent_ref(k["logits"], k["tgt"], V, 1.0)
    _check_dlogits(dl, d, 1.0 / cnt, k["tgt"], V, "lm_head separate dlogits")
    dl64 = dl.double()
    check_banded(h.grad.cpu(), *behind(dl64, None, c["b"] * c["u"], VP), "lm_head dh from the observed dlogits")
    check_banded(w.grad.cpu(), *behind(dl64.t(), None, c["a"], LM_N, m.gemm_dw_splits(LM_N, VP, C) > 1),
                 "lm_head dW from the observed dlogits")
    two = run_lm(ops, dict(_LM_CHUNK=-1, _XENT_FUSED=False))
    assert route_ok(two["names"], ["_LMHeadXentFn"], ["_XentFn"])
    assert same_bits(two["dh"], h.grad.cpu()), "lm_head: the two-kernel chunk route and linear + cross_entropy differ in dh"
    assert same_bits(two["dw"], w.grad.cpu()), "lm_head: the two-kernel chunk route and linear + cross_entropy differ in dW"


def test_lm_head_split_slot(cuda):
    """A split wte: two forwards then two backwards (dloss 0.5 and 0.25) leave RNE(RNE(d1 dW1) + d2 dW2)
    in the head slot, ready fires once, after the second backward; a forward whose graph is dropped
    leaves the slot's bits untouched."""
    ops = _ops()
    k = lm_case()
    c = k["c"]
    h2v = gints((LM_N, C), 111, A_MAX)
    with hooks(_LM_CHUNK=-1):
        w = leaf(c["b"], c["u"])
        dws = []
        for hv in (c["a"], h2v):
            w.grad = None
            ops.lm_head_xent(dev(hv), w, k["tgt"].cuda(), V).backward()
            dws.append(w.grad.detach().cpu().double())
        ar = Arena(split=("wte",), late=("wte",), wte=c["b"] * c["u"])
        sp = ar.wte._pdo_split
        fired = []
        sp.ready = lambda s: fired.append(s.grad.detach().clone())
        hs = [leaf(c["a"]), leaf(h2v)]
        losses = [ops.lm_head_xent(h, ar.wte, k["tgt"].cuda(), V) for h in hs]
        assert_route(losses, ["_LMHeadXentFn"])
        losses[0].backward(torch.tensor(0.5, device="cuda"))
        assert not fired, "the slot was reported ready before the second node had added its part"
        first = (0.5 * dws[0]).to(torch.float32).to(BF16)
        check_bits(sp.grad.detach().cpu(), first, "split slot after the first backward")
        losses[1].backward(torch.tensor(0.25, device="cuda"))
        want = (first.double() + 0.25 * dws[1]).to(torch.float32).to(BF16)
        check_bits(sp.grad.detach().cpu(), want, "split slot after the second backward")
        assert len(fired) == 1 and same_bits(fired[0].cpu(), want)
        assert not bool(ar.wte.grad.any()), "the LM head wrote into the embedding's part of the gradient"
        dropped = ops.lm_head_xent(leaf(c["a"]), ar.wte, k["tgt"].cuda(), V)
        del dropped
        torch.cuda.synchronize()
        check_bits(sp.grad.detach().cpu(), want, "split slot after a dropped forward")
        assert len(fired) == 1
    # outside _LMHeadXentFn's contract (here: chunk 0) the split weight takes _SplitHeadLinearFn, which
    # adds the dW that _LinearFn would return into the slot and signals once
    with hooks(_LM_CHUNK=0):
        plain = run_lm(ops, {})
        assert route_ok(plain["names"], ["_LinearFn", "_XentFn"], ["_SplitHeadLinearFn", "_LMHeadXentFn"])
        ar = Arena(split=("wte",), late=("wte",), wte=c["b"] * c["u"])
        sp, fired = ar.wte._pdo_split, []
        sp.ready = lambda s: fired.append(1)
        r = run_lm(ops, {}, w=ar.wte)
        assert route_ok(r["names"], ["_SplitHeadLinearFn", "_XentFn"], ["_LinearFn", "_LMHeadXentFn"])
        check_bits(sp.grad.detach().cpu(), plain["dw"], "split slot from _SplitHeadLinearFn")
        assert same_bits(r["dh"], plain["dh"]) and r["loss"] == plain["loss"] and fired == [1]
        assert not bool(ar.wte.grad.any()), "_SplitHeadLinearFn wrote into the embedding's part of the gradient"


# ---------------------------------------------------------------------------------------------
# 6. the embedding
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def embed_case():
    """ids in [0, Vp) with long runs of a few ids (they cross 256-row segments once sorted)."""
    B, S = 2, 384
    g = torch.Generator().manual_seed(121)
    idx = torch.where(torch.rand(B, S, generator=g) < 0.8, torch.randint(0, 2, (B, S), generator=g),
                      torch.randint(0, VP, (B, S), generator=g))
    idx.view(-1)[[0, 1]] = torch.tensor([VP - 1, 0])
    return dict(B=B, S=S, idx=idx, dy=randn16((B, S, C), g), base=randn16((VP, C), g, 4.0).to(BF16),
                wte=randn16((VP, C), g), wpe=randn16((S + 2, C), g))


def test_embedding_routes(cuda):
    """Without a split slot _EmbedFn returns RNE(float64 index_add) for integer dy (embed_bwd).  With
    FlatParams(split=("wte",)) it adds straight into wte.grad by embed_bwd_sorted: sorted_reference
    onto the gradient's previous bits, and _pdo_ready fires once."""
    ops, k = _ops(), embed_case()
    B, S, idx = k["B"], k["S"], k["idx"]
    counts = torch.bincount(idx.flatten(), minlength=VP)
    assert int(counts.max()) > 256 and int(counts.max()) * 8 < LIM
    wte, wpe = leaf(k["wte"]), leaf(k["wpe"])
    y = ops.embedding(idx.cuda(), wte, wpe)
    assert_route(y, ["_EmbedFn"])
    check_bits(grad2(y), (k["wte"].float()[idx] + k["wpe"].float()[:S]).to(BF16).reshape(-1, C), "embedding y")
    dyi = gints((B, S, C), 122, 8)
    y.backward(dev(dyi))
    ref = torch.zeros(VP, C, dtype=F64).index_add_(0, idx.flatten(), dyi.reshape(-1, C))
    check_bits(wte.grad, as_bf16(rne(ref)), "embedding dwte (atomic route)")
    ar = Arena(split=("wte",), late=("wte",), wte=k["wte"], wpe=k["wpe"])
    ar.wte.grad.copy_(k["base"].cuda())
    head_before = ar.wte._pdo_split.grad.detach().clone()
    y = ops.embedding(idx.cuda(), ar.wte, ar.wpe)
    assert_route(y, ["_EmbedFn"])
    y.backward(dev(k["dy"]))
    keys, perm = torch.sort(idx.flatten(), stable=True)
    want = sorted_reference(k["dy"].reshape(B * S, C).to(torch.float32), keys, perm, k["base"])
    check_bits(ar.grad("wte"), want, "embedding dwte (sorted route into the arena)")
    assert ar.ready["wte"] == 1
    assert same_bits(ar.wte._pdo_split.grad, head_before), "the embedding wrote into the LM head's slot"


# ---------------------------------------------------------------------------------------------
# 7. one block on random data: arena, wt_scope and deferred reductions give the same bits
# ---------------------------------------------------------------------------------------------
BLOCK_ROUTES = {
    "default": (dict(), ["_LayerNormFn", "_QKVAttnFn", "_LinearResFn", "_LNResFn", "_NTMLPFn"],
                ["_AddLayerNormFn", "_LinearFn", "_BiasGeluFn", "_GeluLinearFn", "_FlashAttnFn"]),
    "unfused": (dict(_RES_EPI=False, _NT_GELU=False, _QKV_FUSED=False),
                ["_LayerNormFn", "_LinearFn", "_FlashAttnFn", "_AddLayerNormFn", "_GeluLinearFn"],
                ["_LinearResFn", "_LNResFn", "_NTMLPFn", "_QKVAttnFn", "_BiasGeluFn"]),
    "kernels": (dict(_RES_EPI=False, _NT_DGELU=False),
                ["_LayerNormFn", "_QKVAttnFn", "_LinearFn", "_AddLayerNormFn", "_BiasGeluFn"],
                ["_LinearResFn", "_LNResFn", "_NTMLPFn", "_GeluLinearFn"]),
}


@functools.lru_cache(maxsize=None)
def block_values(S, batch=0):
    """The block's parameters and one micro-batch (x and the two output gradients); batch 1 holds other
    activations and gradients for the same parameters."""
    if batch:
        g = torch.Generator().manual_seed(977 * batch + S)
        return dict(block_values(S), x=randn16((2, S, C), g), d1=randn16((2, S, C), g), d2=randn16((2, S, C), g))
    g = torch.Generator().manual_seed(131 + S)
    r = lambda *s, sc=1.0: randn16(s, g, sc)   # noqa: E731
    one = lambda: q16(1 + r(C, sc=0.1))        # noqa: E731
    vals = dict(g0=one(), be0=r(C, sc=0.1), wqkv=r(3 * C, C, sc=0.05), bqkv=r(3 * C, sc=0.1),
                wo=r(C, C, sc=0.05), bo=r(C, sc=0.1), g1=one(), be1=r(C, sc=0.1), w1=r(HID, C, sc=0.05),
                b1=r(HID, sc=0.1), w2=r(C, HID, sc=0.03), b2=r(C, sc=0.1), g2=one(), be2=r(C, sc=0.1))
    return dict(vals=vals, x=r(2, S, C), d1=r(2, S, C), d2=r(2, S, C))


def run_block(ops, S, P, scopes=(), batch=0):
    k = block_values(S, batch)
    x = leaf(k["x"])
    with contextlib.ExitStack() as st:
        for s in scopes:
            if s == "wt":
                st.enter_context(P.flat.wt_scope())
        y0 = ops.layer_norm(x, P.g0, P.be0)
        at = ops.qkv_attention(y0, P.wqkv, P.bqkv, HEADS)
        h1, y1 = ops.linear_add_layer_norm(at, P.wo, P.bo, x, P.g1, P.be1)
        h2, y2 = ops.mlp_add_layer_norm(y1, P.w1, P.b1, P.w2, P.b2, h1, P.g2, P.be2)
        names = nodes(h2, y2)
        if "deferred" in scopes:
            st.enter_context(ops.deferred_reductions("cuda"))
        with calls(_m(), "transpose") as n:
            torch.autograd.backward([h2, y2], [dev(k["d1"]), dev(k["d2"])])
        pending = int(_m().colsum_pending())
    ops.flush_deferred()
    assert int(_m().colsum_pending()) == 0
    torch.cuda.synchronize()
    if isinstance(P, Arena):
        # the scopes took effect: column sums were queued (or not), W^T came from the arena (or was built)
        assert (pending > 0) == ("deferred" in scopes), (scopes, pending)
        assert (n["transpose"] == 0) == ("wt" in scopes), (scopes, n)
    return names, h2.detach().cpu(), y2.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("S", (128, 384))
@pytest.mark.parametrize("name", list(BLOCK_ROUTES))
def test_block_routes_give_identical_bits(cuda, name, S):
    """layer_norm -> qkv_attention -> linear_add_layer_norm -> mlp_add_layer_norm on random data: every
    gradient written into a zeroed arena equals the returned-tensor route bit for bit, with the
    prebuilt W^T live (wt_scope) or not, and with the column sums deferred or not."""
    ops = _ops()
    hk, ran, not_ran = BLOCK_ROUTES[name]
    vals = block_values(S)["vals"]
    with hooks(**hk):
        P = Params(**vals)
        names, h2, y2, dx = run_block(ops, S, P)
        assert route_ok(names, ran, not_ran), (name, sorted(names))
        base = {n: getattr(P, n).grad.detach().cpu() for n in vals}
        P2 = Params(**vals)
        run_block(ops, S, P2, batch=1)
        other = {n: getattr(P2, n).grad.detach().cpu() for n in vals}     # the second micro-batch alone
        assert all(bool(torch.isfinite(g.float()).all()) and bool(g.any()) for g in base.values())
        for scopes in ((), ("wt",), ("deferred",), ("wt", "deferred")):
            ar = Arena(**vals)
            if "wt" in scopes:
                ar.flat.enable_wt()
                assert ar.flat.wt is not None
            names_a, h2a, y2a, dxa = run_block(ops, S, ar, scopes)
            assert route_ok(names_a, ran, not_ran), (name, scopes, sorted(names_a))
            what = f"block {name} S={S} scopes {scopes}"
            assert same_bits(h2a, h2) and same_bits(y2a, y2), f"{what}: outputs differ"
            assert same_bits(dxa, dx), f"{what}: dx differs"
            for n in vals:
                assert same_bits(ar.grad(n), base[n]), f"{what}: arena gradient {n} differs from the returned one"
            assert all(v == 1 for v in ar.ready.values()), (what, ar.ready)
            if scopes in ((), ("wt", "deferred")):
                # a second micro-batch with other activations and gradients accumulates onto the first;
                # zero_grad() and the second again gives the second alone
                run_block(ops, S, ar, scopes, batch=1)
                for n in vals:
                    bad = ~accum_ok(base[n], ar.grad(n), other[n])
                    assert not bool(bad.any()), f"{what}: {n} after a second backward is not RNE(first + second) " \
                                                f"in {int(bad.sum())} of {bad.numel()} elements"
                    assert not same_bits(ar.grad(n), other[n]) and not same_bits(ar.grad(n), base[n])
                ar.flat.zero_grad()
                run_block(ops, S, ar, scopes, batch=1)
                for n in vals:
                    assert same_bits(ar.grad(n), other[n]), f"{what}: {n} after zero_grad() is not the second alone"
                assert all(v == 3 for v in ar.ready.values()), (what, ar.ready)
