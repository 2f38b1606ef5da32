"""Bit-exact checks of the implicit-GEMM convolutions (csrc/hip/conv.hip) at tiny, non-square shapes.

Method.  Every kernel here multiplies bf16 operands exactly, accumulates in fp32 and rounds once at
the end.  With small INTEGER inputs every fp32 sum the kernel can form, in any order, is an integer
below 2^24 and therefore exact, so the result does not depend on the summation order, the tile
configuration or the split count, and each output element is known exactly:

  bf16 outputs   the float64 result rounded once to bf16, round-to-nearest-even (the float64 value
                 is an integer < 2^24, so float64 -> float32 is exact and float32 -> bf16 is the one
                 rounding);
  fp32 outputs   the float64 result itself.

The bound K_total * max|a| * max|b| (+ max|addend|) < 2^24 is asserted on the inputs of every case
(exact_bound).  The expected values come from float64 F.conv2d / autograd on the CPU, never from a
kernel; references are computed once per shape and shared unchanged.  Comparisons are on the bit
patterns, and a mismatch is reported at its first differing element in the operation's own
coordinates: (n, h, w, channel) for activations, (kout, r, s, cin) for weights, (tile, channel) for
the tile statistics.  test_conv_exact_cpu.py validates the helpers and tables of this file.

Rounding contracts (read from the epilogues):
  conv_dgrad(add=)   conv_epilogue adds the addend to the fp32 accumulator and converts once:
                     dx = RNE_bf16(fp32 sum + float(add)).  Parity classes without a tap (1x1
                     stride 2) hold the addend's bits verbatim, or +0 without an addend.
  conv_wgrad(out=)   conv_wgrad_reduce adds the fp32 partials to out in fp32: exact for integers.
  conv_stride2_add   RNE_bf16(float(dx) + float(add)) at the pixels (2a, 2b), nothing else touched.
  conv_fwd stats     the per-tile sum adds bf16-rounded outputs (integers) in fp32 through registers,
                     wave shuffles and LDS: integers below 2^24 throughout, hence compared exactly.
                     The centred sum of squares subtracts sum / rows, which is not an integer: it is
                     held to the project's tolerance for per-group partials (rtol = atol = 2e-3).

The weight-gradient dispatch has no query function, so wgrad_plan() repeats the host code
(wgrad_c64_splits, wgrad_dw4_splits, conv_wgrad_dw4_splits, wgrad_cfg, wgrad_fold) and the table
names the path every shape is there for; the CPU file asserts plan == table.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
LIM = 1 << 24
STATS_RTOL = STATS_ATOL = 2e-3  # test_nt_bn_stats_epilogue_vs_fp32's tolerance for per-group partials
NCU = 256  # compute units of an MI355X (conv_wgrad_dw4_splits sizes its splits by them)

# input magnitudes: activations, weights, output gradients, joining gradient / accumulate base
X_MAX, W_MAX, DY_MAX, ADD_MAX = 3, 1, 2, 8


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


# ---------------------------------------------------------------------------------------------
# shape tables: (N, C, H, W, Kout, R, stride), pad = (R - 1) / 2
# ---------------------------------------------------------------------------------------------
SHAPES = [
    (1, 64, 3, 4, 64, 3, 1),      # every pixel touches padding; one partial 256-row tile
    (1, 64, 5, 9, 64, 3, 1),      # 45 tokens: partial last tile of the 256 x 64 configuration
    (3, 64, 7, 7, 128, 3, 1),     # 147 tokens: partial last tile of the 128 x 128 configuration
    (2, 64, 9, 6, 64, 3, 2),      # stride 2, odd H
    (2, 128, 8, 12, 128, 3, 2),   # stride 2, even extents: parity-1 rows want dy row Ho (masked)
    (2, 128, 7, 9, 256, 1, 2),    # 1x1 stride 2: three parity classes without a tap
    (2, 256, 8, 6, 512, 1, 2),    # 1x1 stride 2, even extents
    (1, 512, 4, 5, 512, 3, 1),    # reduction length 4608
    (2, 64, 40, 56, 64, 1, 1),    # 4480 tokens, H != W, neither a power of two: divmods at larger indices
]

# weight-gradient table: (shape, path, why).  path "taps" = the tap-group kernels, "gather" = the
# gathered gemm_dw4 mainloop, "pertap" = the per-tap kernel.  The mode switches a path needs:
WGRAD_MODES = {"taps": (1, 1), "gather": (0, 1), "pertap": (0, 0)}  # (conv_wgrad_c64_mode, conv_wgrad_mode)
WGRAD = [
    ((3, 64, 7, 7, 64, 3, 1), "taps", "C = 64, 147 tokens: partial last 64-token k-step"),
    ((3, 128, 7, 7, 128, 3, 1), "taps", "C = 128, partial last k-step"),
    ((2, 64, 9, 6, 64, 3, 2), "taps", "C = 64, stride 2"),
    ((2, 128, 8, 12, 128, 3, 2), "taps", "C = 128, stride 2"),
    ((4, 64, 16, 20, 64, 3, 1), "taps", "1280 tokens: 5 splits, fold template 4"),
    ((8, 64, 32, 32, 64, 3, 1), "taps", "8192 tokens: 32 splits, fold template 16"),
    ((4, 256, 8, 8, 256, 3, 1), "gather", "the minimum: 256 tokens at one split"),
    ((4, 256, 8, 8, 128, 3, 1), "gather", "half-height Kout = 128"),
    ((4, 128, 8, 8, 256, 3, 1), "gather", "R*S*C = 1152: zero-padded last 256-column tile"),
    ((8, 256, 16, 8, 256, 3, 2), "gather", "stride 2"),
    ((4, 256, 8, 32, 256, 3, 1), "gather", "1024 tokens: 4 splits, fold template 4"),
    ((2, 64, 9, 6, 64, 3, 2), "pertap", "template (64, 64), stride 2"),
    ((3, 64, 7, 7, 128, 3, 1), "pertap", "template (128, 64), partial last k-step"),
    ((2, 128, 6, 10, 64, 3, 1), "pertap", "template (64, 128)"),
    ((2, 128, 7, 9, 256, 1, 2), "pertap", "template (128, 128), 1x1 stride 2"),
    ((2, 64, 40, 56, 64, 1, 1), "pertap", "4480 tokens on one tile: 8 splits, fold template 4"),
    ((8, 64, 32, 32, 64, 3, 1), "pertap", "8192 tokens: 16 splits, fold template 16"),
]
ALL_PATHS = (4, 128, 8, 8, 128, 3, 1)  # C = Kout = 128, 3x3, 256 tokens: every path supports it

STEM_SHAPES = [(1, 8, 14), (3, 30, 30), (2, 12, 20)]  # (N, H, W)
STRIDE2_ADD_SHAPES = [(2, 64, 7, 9), (1, 64, 8, 6)]   # (N, C, H, W)
NEEDLE_SHAPES = [(1, 64, 5, 9, 64, 3, 1), (2, 64, 9, 6, 64, 3, 2)]


def sid(shape):
    return "x".join(str(v) for v in shape)


def geometry(shape):
    N, C, H, W, K, R, st = shape
    pad = (R - 1) // 2
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1
    return pad, Ho, Wo, N * Ho * Wo


def fold_template(splits, rows, cols):
    """conv_wgrad_reduce_kernel's template wgrad_fold picks."""
    n4 = rows * cols // 4
    return 16 if splits >= 16 and n4 < 1024 * 64 else 4 if splits >= 4 else 1


def wgrad_plan(shape, c64_mode, dw4_mode, ncu=NCU):
    """conv_wgrad_nhwc's dispatch for a shape under the two mode switches: path, splits, fold template."""
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, M = geometry(shape)
    ks, TC = (M + 63) // 64, R * R * C
    if c64_mode and C == K and C in (64, 128) and R == 3:
        sp = max(1, min(256 if C == 64 else 85, ks // 4))
        return dict(path="taps", splits=sp, fold=fold_template(sp, C, 9 * C))
    if dw4_mode and K % 128 == 0 and TC % 128 == 0 and C % 8 == 0 and M % 128 == 0 and \
            not (R == 1 and st == 1 and (K % 256 or C % 256)):
        tiles = ((K + 255) // 256) * ((TC + 255) // 256)
        sp = max(1, min(ncu // tiles, (M // 128) // 2, 256))
        if (M // 128) // sp >= 2:
            return dict(path="gather", splits=sp, fold=fold_template(sp, K, TC))
    bm, bn = 128 if K % 128 == 0 else 64, 128 if C % 128 == 0 else 64
    tiles = (K // bm) * (R * R * C // bn)
    sp = max(1, min((512 + tiles - 1) // tiles, ks // 8, 256))
    return dict(path="pertap", splits=sp, fold=fold_template(sp, K, TC), bm=bm, bn=bn)


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def first_mismatch(got, want, names):
    """None when got and want have the same bits; else a description of the first differing element
    (row-major order of the view handed in), its index spelled in `names`."""
    assert got.dtype == want.dtype, f"dtype {got.dtype} vs {want.dtype}"
    assert got.shape == want.shape, f"shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert len(names) == got.dim()
    ne = _bits(got) != _bits(want)
    count = int(ne.sum())
    if count == 0:
        return None
    flat = int(ne.reshape(-1).nonzero()[0])
    idx = []
    for d in reversed(got.shape):
        idx.append(flat % d)
        flat //= d
    idx = tuple(reversed(idx))
    where = ", ".join(f"{n} {i}" for n, i in zip(names, idx))
    return f"first mismatch at {where}: got {float(got[idx])!r}, expected {float(want[idx])!r} " \
           f"({count} of {got.numel()} elements differ)"


NHWC = ("n", "h", "w", "channel")
KRSC = ("kout", "r", "s", "cin")


def nhwc(t):
    """[N, C, H, W] (any memory format) viewed as [N, H, W, C]; the same view turns a weight
    [K, C, R, S] into [K, R, S, C]."""
    return t.permute(0, 2, 3, 1)


def check_bits(got, want, names, what):
    msg = first_mismatch(got.cpu(), want.cpu(), names)
    assert msg is None, f"{what}: {msg}"


# ---------------------------------------------------------------------------------------------
# inputs and float64 references (CPU)
# ---------------------------------------------------------------------------------------------
def ints(shape, amax, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amax, amax + 1, shape, generator=g).to(F64)


def exact_bound(k_total, amax, bmax, extra=0):
    """The largest magnitude any partial sum of k_total products (plus an addend) can reach."""
    return k_total * amax * bmax + extra


def rne_bf16(t):
    """float64 integers below 2^24 rounded once to bf16 (float64 -> float32 is exact for them)."""
    assert bool((t == t.round()).all()) and float(t.abs().max()) < LIM
    return (t + 0.0).to(torch.float32).to(BF16)  # + 0.0: a sum of -0 products is +0 in the kernels


def exact_f32(t):
    assert bool((t == t.round()).all()) and float(t.abs().max()) < LIM
    return (t + 0.0).to(torch.float32)


def conv_ref(x, w, stride):
    return F.conv2d(x, w, stride=stride, padding=(w.shape[-1] - 1) // 2)


def grads_ref(x, w, dy, stride):
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    dx, dw = torch.autograd.grad(conv_ref(xr, wr, stride), (xr, wr), dy)
    return dx, dw


def tile_stats_ref(rows, tile):
    """[tiles, 2, K] float64: per tile of `tile` rows of rows [M, K] (the last one partial) the sum
    and the sum of squares about the tile's own mean, over exactly the tile's valid rows."""
    M, K = rows.shape
    out = torch.zeros((M + tile - 1) // tile, 2, K, dtype=F64)
    for i in range(out.shape[0]):
        r = rows[i * tile:min(M, (i + 1) * tile)]
        out[i, 0] = r.sum(0)
        out[i, 1] = ((r - r.mean(0)) ** 2).sum(0)
    return out


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs and float64 references of one convolution shape (CPU, shared, never modified)."""
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, M = geometry(shape)
    seed = sum(v * 31 ** i for i, v in enumerate(shape)) % (1 << 31)
    x, w = ints((N, C, H, W), X_MAX, seed), ints((K, C, R, R), W_MAX, seed + 1)
    dy, add = ints((N, K, Ho, Wo), DY_MAX, seed + 2), ints((N, C, H, W), ADD_MAX, seed + 3)
    base = ints((K, C, R, R), ADD_MAX, seed + 4)
    # every fp32 sum a kernel can form is an integer below 2^24: K_total * max|a| * max|b| (+ addend)
    assert exact_bound(R * R * C, X_MAX, W_MAX) < LIM                   # forward, and its tile sums below
    assert 256 * exact_bound(R * R * C, X_MAX, W_MAX) < LIM             # sum over a tile of <= 256 rows
    assert exact_bound(R * R * K, DY_MAX, W_MAX, ADD_MAX) < LIM         # input gradient (+ add)
    assert exact_bound(M, DY_MAX, X_MAX, ADD_MAX) < LIM                 # weight gradient (+ out)
    for t, amax in ((x, X_MAX), (w, W_MAX), (dy, DY_MAX), (add, ADD_MAX), (base, ADD_MAX)):
        assert float(t.abs().max()) <= amax and bool((t == t.round()).all())
    y = conv_ref(x, w, st)
    dx, dw = grads_ref(x, w, dy, st)
    return dict(x=x, w=w, dy=dy, add=add, base=base, y=y, dx=dx, dw=dw)


def dev_bf16(t):
    """An integer float64 CPU tensor as a fresh channels_last bf16 device tensor."""
    return t.to(BF16).cuda().contiguous(memory_format=torch.channels_last)


def dev_f32(t):
    return t.to(torch.float32).cuda().contiguous(memory_format=torch.channels_last)


def record(line):
    """One line for the results file (profiles/r9_conv_dw_exact_tests.md is written from these)."""
    print(f"[exact] {line}")


# ---------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------
def check_tile_stats(st, y, K, tile, what):
    """Tile statistics against float64 sums of the kernel's own bf16 output over each tile's valid rows."""
    rows = nhwc(y).reshape(-1, K).cpu().to(F64)
    ref = tile_stats_ref(rows, tile)
    assert st.shape == ref.shape and st.dtype == torch.float32, f"{what}: stats {tuple(st.shape)}"
    got = st.cpu()
    check_bits(got[:, 0], exact_f32(ref[:, 0]), ("tile", "channel"), f"{what}: tile sums")
    ratio = (got[:, 1].to(F64) - ref[:, 1]).abs() / (STATS_ATOL + STATS_RTOL * ref[:, 1].abs())
    worst = float(ratio.max())
    record(f"{what}: centred sum of squares, worst |err| / (atol + rtol |ref|) = {worst:.3e}")
    if worst > 1.0:
        t, c = divmod(int(ratio.argmax()), K)
        raise AssertionError(f"{what}: centred sum of squares at tile {t}, channel {c}: got "
                             f"{float(got[t, 1, c])!r}, float64 {float(ref[t, 1, c])!r}, ratio {worst:.3f}")
    return worst


@pytest.mark.parametrize("with_stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_conv_fwd_exact(shape, with_stats):
    """conv_fwd: y bit-equal to the float64 convolution rounded once to bf16; with statistics, each
    tile's sum exactly the sum of the kernel's own output over that tile's valid rows (fp32 sums of
    integers below 2^24 stay exact), its centred sum of squares within rtol = atol = 2e-3."""
    m, c = _m(), case(shape)
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, M = geometry(shape)
    assert m.conv_ok(N, H, W, C, K, R, R, st, pad)
    y, stats = m.conv_fwd(dev_bf16(c["x"]), dev_bf16(c["w"]), st, pad, with_stats)
    assert y.shape == (N, K, Ho, Wo) and y.is_contiguous(memory_format=torch.channels_last)
    check_bits(nhwc(y), nhwc(rne_bf16(c["y"])), NHWC, f"conv_fwd {sid(shape)}")
    if with_stats:
        tile = m.conv_tile_rows(K)
        assert tile == (256 if K == 64 else 128)
        record(f"conv_fwd {sid(shape)}: {M} tokens, {tile}-row tiles x {(M + tile - 1) // tile}")
        check_tile_stats(stats, y, K, tile, f"conv_fwd {sid(shape)}")


# ---------------------------------------------------------------------------------------------
# 2. / 3. input gradient
# ---------------------------------------------------------------------------------------------
def _poison(shape):
    """A NaN-filled block of dx's size, freed again: the allocator tends to hand it to the next
    at::empty of that size, so an element the kernel leaves unwritten is unlikely to read as zero."""
    junk = torch.full(shape, float("nan"), dtype=BF16, device="cuda")
    del junk


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_conv_dgrad_exact(shape):
    """conv_dgrad: dx bit-equal to float64 autograd rounded once, every element written (the parity
    classes of a 1x1 stride-2 convolution that no tap reaches are +0); with add=, dx =
    RNE_bf16(fp32 sum + add) — one rounding — and those classes hold the addend verbatim."""
    m, c = _m(), case(shape)
    N, C, H, W, K, R, st = shape
    pad = geometry(shape)[0]
    w, dy, add = dev_bf16(c["w"]), dev_bf16(c["dy"]), dev_bf16(c["add"])
    wt = m.conv_weight_t(w)
    want_wt = c["w"].permute(1, 2, 3, 0).reshape(C, R * R * K).to(BF16)  # [C][tap][K]
    check_bits(wt, want_wt, ("cin", "tap*K + kout"), f"conv_weight_t {sid(shape)}")
    _poison((N, C, H, W))
    dx = m.conv_dgrad(dy, wt, C, R, R, H, W, st, pad)
    assert dx.shape == (N, C, H, W) and dx.is_contiguous(memory_format=torch.channels_last)
    check_bits(nhwc(dx), nhwc(rne_bf16(c["dx"])), NHWC, f"conv_dgrad {sid(shape)}")
    _poison((N, C, H, W))
    dxa = m.conv_dgrad(dy, wt, C, R, R, H, W, st, pad, add)
    check_bits(nhwc(dxa), nhwc(rne_bf16(c["dx"] + c["add"])), NHWC, f"conv_dgrad(add) {sid(shape)}")
    if R == 1 and st == 2:
        zero = torch.zeros((), dtype=BF16)
        for name, sl in (("odd rows", (slice(None), slice(None), slice(1, None, 2))),
                         ("odd columns", (slice(None), slice(None), slice(None), slice(1, None, 2)))):
            got, gota = dx[sl].cpu(), dxa[sl].cpu()
            check_bits(nhwc(got), nhwc(zero.expand_as(got)), NHWC, f"conv_dgrad {sid(shape)}: {name} must be +0")
            check_bits(nhwc(gota), nhwc(c["add"][sl].to(BF16)), NHWC,
                       f"conv_dgrad(add) {sid(shape)}: {name} must be the addend")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_conv_dgrad_bn_dx_exact(shape):
    """conv_dgrad_bn's dx has conv_dgrad's bits on the same inputs (and so the exact ones); the
    partials are test_conv_dgrad_bn_partials' business."""
    m, c = _m(), case(shape)
    N, C, H, W, K, R, st = shape
    pad = geometry(shape)[0]
    dy, wt = dev_bf16(c["dy"]), m.conv_weight_t(dev_bf16(c["w"]))
    ones, zeros = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    dx, part = m.conv_dgrad_bn(dy, wt, R, R, st, pad, dev_bf16(c["x"]), zeros, ones, ones.clone(), zeros.clone(), True)
    plain = m.conv_dgrad(dy, wt, C, R, R, H, W, st, pad)
    check_bits(nhwc(dx), nhwc(plain), NHWC, f"conv_dgrad_bn vs conv_dgrad {sid(shape)}")
    check_bits(nhwc(dx), nhwc(rne_bf16(c["dx"])), NHWC, f"conv_dgrad_bn {sid(shape)}")
    assert part.shape[1:] == (2, C) and bool(torch.isfinite(part).all())


# ---------------------------------------------------------------------------------------------
# 4. conv_stride2_add
# ---------------------------------------------------------------------------------------------
def stride2_add_ref(dx, add):
    """dx, add: float64 values of bf16 tensors.  Expected bf16: RNE(dx + add) at (2a, 2b), dx elsewhere."""
    out = dx.clone()
    out[:, :, ::2, ::2] = dx[:, :, ::2, ::2] + add
    return out.to(torch.float32).to(BF16)


@pytest.mark.parametrize("N,C,H,W", STRIDE2_ADD_SHAPES)
def test_conv_stride2_add_exact(N, C, H, W):
    """dx[n][2a][2b] = RNE_bf16(float(dx) + float(add)), integers up to 300 so that the sums need the
    rounding; every other pixel carries a non-integer sentinel and keeps its bits."""
    m = _m()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dx = ints((N, C, H, W), 300, 5).to(BF16).to(F64)
    add = ints((N, C, Ho, Wo), 300, 6).to(BF16).to(F64)
    assert exact_bound(1, 304, 1, 304) < LIM  # the fp32 sum of two bf16 integers is exact
    sentinel = -0.5 - (torch.arange(N * C * H * W, dtype=F64).reshape(N, C, H, W) % 97)
    keep = torch.ones(H, W, dtype=torch.bool)
    keep[::2, ::2] = False
    dx[:, :, keep] = sentinel[:, :, keep]
    want = stride2_add_ref(dx, add)
    assert bool((want[:, :, keep].to(F64) == sentinel[:, :, keep]).all())  # sentinels are bf16-exact
    got = dev_bf16(dx)
    m.conv_stride2_add(got, dev_bf16(add))
    check_bits(nhwc(got), nhwc(want), NHWC, f"conv_stride2_add {(N, C, H, W)}")


# ---------------------------------------------------------------------------------------------
# 5. weight gradient
# ---------------------------------------------------------------------------------------------
def run_wgrad(m, c, shape, path, out=None):
    N, C, H, W, K, R, st = shape
    pad = geometry(shape)[0]
    c64, dw4 = WGRAD_MODES[path]
    p64, p4 = m.conv_wgrad_c64_mode(c64), m.conv_wgrad_mode(dw4)
    try:
        args = (dev_bf16(c["dy"]), dev_bf16(c["x"]), R, R, st, pad)
        return m.conv_wgrad(*args) if out is None else m.conv_wgrad(*args, out=out)
    finally:
        m.conv_wgrad_c64_mode(p64)
        m.conv_wgrad_mode(p4)


@pytest.mark.parametrize("shape,path,why", WGRAD, ids=[f"{p}-{sid(s)}" for s, p, _ in WGRAD])
def test_conv_wgrad_exact(shape, path, why):
    """conv_wgrad on each of its three paths: the fp32 result is the exact integer, fresh and added
    to an integer fp32 `out` (the fold adds partials and out in fp32: exact below 2^24)."""
    m, c = _m(), case(shape)
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, M = geometry(shape)
    assert m.conv_ok(N, H, W, C, K, R, R, st, pad)
    plan = wgrad_plan(shape, *WGRAD_MODES[path], ncu=torch.cuda.get_device_properties(0).multi_processor_count)
    assert plan["path"] == path, f"{sid(shape)} was listed for {path} but dispatches to {plan}"
    record(f"conv_wgrad {sid(shape)} ({why}): {M} tokens, {plan}")
    dw = run_wgrad(m, c, shape, path)
    assert dw.shape == (K, C, R, R) and dw.dtype == torch.float32
    check_bits(nhwc(dw), nhwc(exact_f32(c["dw"])), KRSC, f"conv_wgrad[{path}] {sid(shape)}")
    acc = dev_f32(c["base"])
    ret = run_wgrad(m, c, shape, path, out=acc)
    assert ret.data_ptr() == acc.data_ptr()
    check_bits(nhwc(acc), nhwc(exact_f32(c["dw"] + c["base"])), KRSC, f"conv_wgrad[{path}](out=) {sid(shape)}")


def test_conv_wgrad_paths_agree():
    """Tap-group, gathered and per-tap kernels on one shape all three support: the same bits."""
    m, c = _m(), case(ALL_PATHS)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    res = {}
    for path in ("taps", "gather", "pertap"):
        plan = wgrad_plan(ALL_PATHS, *WGRAD_MODES[path], ncu=ncu)
        assert plan["path"] == path, plan
        record(f"conv_wgrad paths agree {sid(ALL_PATHS)}: {plan}")
        res[path] = run_wgrad(m, c, ALL_PATHS, path)
        check_bits(nhwc(res[path]), nhwc(exact_f32(c["dw"])), KRSC, f"conv_wgrad[{path}] {sid(ALL_PATHS)}")
    check_bits(nhwc(res["taps"]), nhwc(res["gather"]), KRSC, "tap-group vs gathered")
    check_bits(nhwc(res["taps"]), nhwc(res["pertap"]), KRSC, "tap-group vs per-tap")


# ---------------------------------------------------------------------------------------------
# binding checks: a dy that does not match (N, Kout, Ho, Wo) raises before any launch
# ---------------------------------------------------------------------------------------------
def test_conv_gradient_bindings_reject_mismatched_dy():
    m = _m()
    shape = (2, 64, 9, 6, 64, 3, 2)
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, M = geometry(shape)
    c = case(shape)
    x, wt = dev_bf16(c["x"]), m.conv_weight_t(dev_bf16(c["w"]))
    ones, zeros = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")

    def dy_of(n, k, h, w):
        return torch.zeros(n, k, h, w, dtype=BF16, device="cuda").contiguous(memory_format=torch.channels_last)

    bad = {"batch": dy_of(N + 1, K, Ho, Wo), "rows": dy_of(N, K, Ho + 1, Wo), "columns": dy_of(N, K, Ho, Wo - 1),
           "stride-1 extent": dy_of(N, K, H, W)}
    for name, dy in bad.items():
        with pytest.raises(RuntimeError, match="conv_wgrad"):
            m.conv_wgrad(dy, x, R, R, st, pad)
        if name != "batch":  # conv_dgrad has no second tensor to take a batch from: dx gets dy's
            with pytest.raises(RuntimeError, match="conv_dgrad"):
                m.conv_dgrad(dy, wt, C, R, R, H, W, st, pad)
        with pytest.raises(RuntimeError, match="conv_dgrad_bn"):
            m.conv_dgrad_bn(dy, wt, R, R, st, pad, x, zeros, ones, ones, zeros, True)
    good = dy_of(N, K, Ho, Wo)
    # channel counts: a weight transpose for other channels, an x with other channels than `out`
    with pytest.raises(RuntimeError, match="conv_dgrad"):
        m.conv_dgrad(dy_of(N, 128, Ho, Wo), wt, C, R, R, H, W, st, pad)
    with pytest.raises(RuntimeError, match="conv_wgrad"):
        m.conv_wgrad(good, x, R, R, st, pad, out=torch.zeros(K, 2 * C, R, R, device="cuda"))
    # unsupported geometry (48 channels, a 5x5 kernel, stride 3) is an error before anything is allocated
    x48 = torch.zeros(N, 48, H, W, dtype=BF16, device="cuda").contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="unsupported"):
        m.conv_wgrad(good, x48, R, R, st, pad)
    with pytest.raises(RuntimeError, match="unsupported"):
        m.conv_wgrad(good, x, 5, 5, st, 2)
    with pytest.raises(RuntimeError, match="unsupported"):
        m.conv_dgrad(good, wt, C, R, R, H, W, 3, pad)
    with pytest.raises(RuntimeError, match="unsupported"):
        m.conv_dgrad_bn(good, wt, R, R, 3, pad, x, zeros, ones, ones, zeros, True)
    # and the matching call still works
    assert m.conv_wgrad(good, x, R, R, st, pad).shape == (K, C, R, R)
    assert m.conv_dgrad(good, wt, C, R, R, H, W, st, pad).shape == (N, C, H, W)


# ---------------------------------------------------------------------------------------------
# 6. stem
# ---------------------------------------------------------------------------------------------
def s2d_ref(x):
    """z[n][(2p + q)*3 + c][i][j] = x[n][c][2i + p][2j + q], channels 12-15 zero ([N, 16, H/2, W/2])."""
    N, C, H, W = x.shape
    z = torch.zeros(N, 16, H // 2, W // 2, dtype=x.dtype)
    for p in range(2):
        for q in range(2):
            z[:, (2 * p + q) * 3:(2 * p + q) * 3 + 3] = x[:, :, p::2, q::2]
    return z


@functools.lru_cache(maxsize=None)
def stem_case(N, H, W):
    x, w = ints((N, 3, H, W), X_MAX, 7 * H + W), ints((64, 3, 7, 7), W_MAX, 7 * H + W + 1)
    dy, base = ints((N, 64, H // 2, W // 2), DY_MAX, 7 * H + W + 2), ints((64, 3, 7, 7), ADD_MAX, 7 * H + W + 3)
    assert exact_bound(147, X_MAX, W_MAX) < LIM
    assert exact_bound(N * (H // 2) * (W // 2), DY_MAX, X_MAX, ADD_MAX) < LIM
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = F.conv2d(xr, wr, stride=2, padding=3)
    dw, = torch.autograd.grad(y, (wr,), dy)
    return dict(x=x, w=w, dy=dy, base=base, y=y.detach(), dw=dw, z=s2d_ref(x))


@pytest.mark.parametrize("N,H,W", STEM_SHAPES)
def test_stem_exact(N, H, W):
    """stem_fwd: z the exact space-to-depth permutation of x (bitwise), y bit-equal to the float64
    7x7 / stride 2 / pad 3 convolution rounded once; stem_wgrad: the exact integers, fresh and
    added to an integer fp32 out (stem_dw_kernel adds in fp32)."""
    m, c = _m(), stem_case(N, H, W)
    assert m.stem_ok(N, H, W, 3, 64)
    y, st, z = m.stem_fwd(dev_bf16(c["x"]), dev_bf16(c["w"]), True)
    what = f"stem {(N, H, W)}"
    check_bits(nhwc(z), nhwc(c["z"].to(BF16)), NHWC, f"{what}: z")
    check_bits(nhwc(y), nhwc(rne_bf16(c["y"])), NHWC, f"{what}: y")
    check_tile_stats(st, y, 64, m.stem_tile_rows(), what)
    dy = dev_bf16(c["dy"])
    dw = m.stem_wgrad(dy, z)
    assert dw.shape == (64, 3, 7, 7) and dw.dtype == torch.float32
    check_bits(nhwc(dw), nhwc(exact_f32(c["dw"])), KRSC, f"{what}: dw")
    acc = dev_f32(c["base"])
    m.stem_wgrad(dy, z, acc)
    check_bits(nhwc(acc), nhwc(exact_f32(c["dw"] + c["base"])), KRSC, f"{what}: dw accumulated")


# ---------------------------------------------------------------------------------------------
# 7. needles
# ---------------------------------------------------------------------------------------------
def needle_pixels(N, H, W):
    """The four corners and the centre of every image with distinct values 1 .. 5."""
    return [(n, h, w, v) for n in range(N)
            for v, (h, w) in enumerate([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)], 1)]


def needle_weight(K, C, R):
    """w[k][c][r][s] = (tap + 1) + 9 * ((k + c) % 5): distinct per tap, and per channel within five."""
    k, c = torch.arange(K).view(K, 1, 1, 1), torch.arange(C).view(1, C, 1, 1)
    tap = (torch.arange(R).view(R, 1) * R + torch.arange(R).view(1, R)).view(1, 1, R, R)
    return ((tap + 1) + 9 * ((k + c) % 5)).to(F64)


def needle_fwd_ref(shape, ch):
    """Forward of the needle input (needles in channel `ch`) by placing taps: float64 y, and per
    output pixel the (needle value, r, s) taps that reach it."""
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, _ = geometry(shape)
    w = needle_weight(K, C, R)
    y, taps = torch.zeros(N, K, Ho, Wo, dtype=F64), {}
    for n, h, wi, v in needle_pixels(N, H, W):
        for r in range(R):
            for s in range(R):
                ho, wo = h + pad - r, wi + pad - s
                if ho % st or wo % st or not (0 <= ho // st < Ho and 0 <= wo // st < Wo):
                    continue
                y[n, :, ho // st, wo // st] += v * w[:, ch, r, s]
                taps.setdefault((n, ho // st, wo // st), []).append((v, r, s))
    return y, taps


def needle_dgrad_ref(shape, ch):
    """Input gradient of a needle dy (needles in output channel `ch`): dx, and the taps per input pixel."""
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, _ = geometry(shape)
    w = needle_weight(K, C, R)
    dx, taps = torch.zeros(N, C, H, W, dtype=F64), {}
    for n, ho, wo, v in needle_pixels(N, Ho, Wo):
        for r in range(R):
            for s in range(R):
                h, wi = ho * st - pad + r, wo * st - pad + s
                if not (0 <= h < H and 0 <= wi < W):
                    continue
                dx[n, :, h, wi] += v * w[ch, :, r, s]
                taps.setdefault((n, h, wi), []).append((v, r, s))
    return dx, taps


def needle_input(N, C, H, W, ch):
    t = torch.zeros(N, C, H, W, dtype=F64)
    for n, h, w, v in needle_pixels(N, H, W):
        t[n, ch, h, w] = v
    return t


def check_needles(got, want, taps, what):
    msg = first_mismatch(nhwc(got).cpu(), nhwc(want), NHWC)
    if msg is None:
        return
    ne = (_bits(nhwc(got).cpu()) != _bits(nhwc(want))).any(-1).nonzero()[0].tolist()
    raise AssertionError(f"{what}: {msg}; pixel {tuple(ne)} expects the (needle value, r, s) taps "
                         f"{taps.get(tuple(ne), 'none: it must be zero')}")


@pytest.mark.parametrize("shape", NEEDLE_SHAPES, ids=sid)
def test_conv_needles(shape):
    """x (dy) zero but for one element at each image corner and the centre, distinct values, and a
    weight that differs per tap: forward and input gradient place exactly the expected taps, so a
    padding or tap-orientation fault reads off the message."""
    m = _m()
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, _ = geometry(shape)
    ch = 37
    w = needle_weight(K, C, R)
    assert float(w.max()) * 5 <= 256 and exact_bound(4, 5, float(w.max())) < LIM  # products bf16-exact
    wd = dev_bf16(w)
    y_ref, taps = needle_fwd_ref(shape, ch)
    y, _ = m.conv_fwd(dev_bf16(needle_input(N, C, H, W, ch)), wd, st, pad, False)
    check_needles(y, rne_bf16(y_ref), taps, f"needles forward {sid(shape)}")
    dx_ref, taps = needle_dgrad_ref(shape, ch)
    dx = m.conv_dgrad(dev_bf16(needle_input(N, K, Ho, Wo, ch)), m.conv_weight_t(wd), C, R, R, H, W, st, pad)
    check_needles(dx, rne_bf16(dx_ref), taps, f"needles dgrad {sid(shape)}")
