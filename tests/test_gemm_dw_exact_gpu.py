"""Bit-exact checks of the weight-gradient GEMM out[M][N] (+)= dy^T x (gemm_dw.hip, gemm_dw4.hip).

dy [T, M] and x [T, N] are integer-valued bf16, so every product is an integer and every fp32 sum the
kernels can form, in any order, is an integer below 2^24 (asserted: T * max|dy| * max|x| + max|base|
< 2^24): the fp32 accumulators are exact whatever the tile, wave or MFMA shape.  The expected output
is the float64 matmul on the CPU, rounded once to bf16 (round-to-nearest-even).

Rounding contract (read from the epilogues).  One split: the kernels add the accumulate base to the
fp32 accumulator and convert once, out = RNE_bf16(base + sum).  Several splits: each split's partial
is rounded to bf16 into the workspace, then splitk_add sums base and partials in fp32 and converts
once.  The partials' rounding is part of the design, so the any-split-count test uses inputs whose
every partial sum over ANY token subset is bf16-exact: each dy column has at most 32 non-zero tokens
of magnitude <= 2 against |x| <= 4, so |partial| <= 256, where bf16 holds every integer.  Then
out = RNE_bf16(base + exact) for every split count, and the non-zeros are placed so that every
(16-token k-step, 128-column block of dy) holds one: a k-step dropped or doubled by any wave of any
split changes the result.

A mismatch is reported at its first element as (tile row, tile column, row and column in the
256 x 256 tile).  test_conv_exact_cpu.py validates the builders and preconditions of this file.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
LIM = 1 << 24
IMPLS = (0, 1, 2)  # gemm_dw_impl: the 8-wave loop, gemm_dw4 on 16x16x32 MFMAs, gemm_dw4 on 32x32x16
V_MAX, BASE_MAX = 4, 8          # dense operands, accumulate base
SPARSE_NNZ, SPARSE_MAX = 32, 2  # per dy column: non-zero tokens, their magnitude

# (T, M, N)
DENSE = [
    (256, 256, 256),     # the shortest legal pipeline of gemm_dw4: two k-tile pairs
    (384, 256, 512),
    (640, 128, 256),     # a half-height tile row alone
    (1280, 384, 512),
    (192, 256, 256),     # T / 64 odd: gemm_dw4 declines, the 8-wave loop runs
    (1024, 50304, 256),  # the LM head's row count and stride at small T
    (65536, 256, 256),   # long k offsets
]
# (T, M, N, impls, forced split counts): each inside the mainloop's contract — gemm_dw4: T % 128 == 0
# and >= 2 k-tile pairs per split; the 8-wave loop: splits <= T / 64, M % 256 == 0; both: <= 16
SPLIT = [
    (1280, 384, 512, (1, 2), (1, 2, 3, 5)),  # 10 pairs dealt 5+5, 4+3+3, 2x5; 3 splits x 4 tiles: remap remainder
    (4096, 256, 256, (0, 1, 2), (16,)),
    (2048, 640, 256, (1, 2), (4,)),          # half-height row plus splits
    (1024, 256, 512, (0,), (1, 3, 16)),
]
# (T, M, N, why)
UNSUPPORTED = [
    (1000, 256, 256, "T % 64 != 0"),
    (256, 256, 128, "N % 256 != 0"),
    (256, 192, 256, "M % 128 != 0"),
    (192, 384, 256, "M % 256 == 128 with odd T / 64"),
]


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def first_mismatch(got, want):
    """None, or the first differing element of an [M, N] output in tile coordinates."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    ne = _bits(got) != _bits(want)
    count = int(ne.sum())
    if count == 0:
        return None
    m, n = divmod(int(ne.reshape(-1).nonzero()[0]), got.shape[1])
    return f"first mismatch at tile ({m // 256}, {n // 256}) row {m % 256} column {n % 256} (m {m}, n {n}): got " \
           f"{float(got[m, n])!r}, expected {float(want[m, n])!r} ({count} of {got.numel()} elements differ)"


def check_bits(got, want, what):
    msg = first_mismatch(got.cpu(), want)
    assert msg is None, f"{what}: {msg}"


def ints(shape, amax, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amax, amax + 1, shape, generator=g, dtype=torch.int8)


def rne_bf16(t):
    """float64 integers below 2^24 rounded once to bf16 (float64 -> float32 is exact for them)."""
    assert bool((t == t.round()).all()) and float(t.abs().max()) < LIM
    return (t + 0.0).to(torch.float32).to(BF16)


def matmul_ref(dy, x):
    """dy^T x in float64 (plain matmul on the CPU)."""
    return dy.to(F64).t() @ x.to(F64)


def sparse_dy(T, M, seed):
    """int8 [T, M]: column m has SPARSE_NNZ non-zeros in {-2, -1, 1, 2}, one in each of the 16-token
    k-steps (32 * (m % 128) + i) % (T / 16), i < 32, at a seeded token of the step — so the 128 columns
    of a block cover every k-step (128 * 32 slots >= T / 16 steps for T <= 65536)."""
    steps = T // 16
    assert T % 16 == 0 and SPARSE_NNZ <= steps <= 128 * SPARSE_NNZ
    g = torch.Generator().manual_seed(seed)
    m = torch.arange(M).view(M, 1)
    step = (SPARSE_NNZ * (m % 128) + torch.arange(SPARSE_NNZ).view(1, -1)) % steps       # [M, 32], distinct per row
    tok = 16 * step + torch.randint(0, 16, step.shape, generator=g)
    val = torch.randint(1, SPARSE_MAX + 1, step.shape, generator=g) * (2 * torch.randint(0, 2, step.shape, generator=g) - 1)
    dy = torch.zeros(T, M, dtype=torch.int8)
    dy[tok.reshape(-1), m.expand_as(tok).reshape(-1)] = val.to(torch.int8).reshape(-1)
    return dy


def sparse_ok(dy):
    """The two properties the any-split test rests on: (<= 32 non-zeros of magnitude <= 2 per column,
    every (16-token k-step, 128-column block) holds a non-zero)."""
    T, M = dy.shape
    nz = dy != 0
    bounded = int(nz.sum(0).max()) <= SPARSE_NNZ and int(dy.abs().max()) <= SPARSE_MAX
    covered = bool(nz.view(T // 16, 16, M // 128, 128).any(3).any(1).all())
    return bounded, covered


@functools.lru_cache(maxsize=None)
def dense_case(T, M, N):
    seed = (T * 7 + M * 3 + N) % (1 << 31)
    dy, x, base = ints((T, M), V_MAX, seed), ints((T, N), V_MAX, seed + 1), ints((M, N), BASE_MAX, seed + 2)
    assert T * V_MAX * V_MAX + BASE_MAX < LIM  # every fp32 sum is an integer below 2^24
    assert int(dy.abs().max()) <= V_MAX and int(x.abs().max()) <= V_MAX and int(base.abs().max()) <= BASE_MAX
    ref = matmul_ref(dy, x)
    return dict(dy=dy, x=x, base=base, fresh=rne_bf16(ref), acc=rne_bf16(ref + base.to(F64)))


@functools.lru_cache(maxsize=None)
def sparse_case(T, M, N):
    seed = (T * 5 + M * 11 + N) % (1 << 31)
    dy, x, base = sparse_dy(T, M, seed), ints((T, N), V_MAX, seed + 1), ints((M, N), BASE_MAX, seed + 2)
    bounded, covered = sparse_ok(dy)
    assert bounded and covered
    assert SPARSE_NNZ * SPARSE_MAX * V_MAX <= 256      # any partial over any token subset is bf16-exact
    assert T * SPARSE_MAX * V_MAX + BASE_MAX < LIM
    ref = matmul_ref(dy, x)
    assert float(ref.abs().max()) <= 256
    return dict(dy=dy, x=x, base=base, fresh=rne_bf16(ref), acc=rne_bf16(ref + base.to(F64)))


def dev(t):
    return t.to(torch.float32).to(BF16).cuda()


def record(line):
    print(f"[exact] {line}")


def run(m, c, ops, accumulate, splits, what):
    """One gemm_dw call on the device operands ops = (dy, x); a non-accumulating call starts from a
    NaN-filled out (every element written)."""
    out = dev(c["base"]) if accumulate else torch.full(c["base"].shape, float("nan"), dtype=BF16, device="cuda")
    assert m.gemm_dw(ops[0], ops[1], out, accumulate, splits), f"{what}: gemm_dw declined"
    check_bits(out, c["acc"] if accumulate else c["fresh"], what)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("T,M,N", DENSE)
def test_gemm_dw_dense_one_split(T, M, N, impl):
    """Dense integer operands in [-4, 4] at one split on each mainloop: out = RNE_bf16(base + exact),
    accumulate off (out pre-filled with NaN) and on.  Half-height shapes (M % 256 == 128) exist on
    gemm_dw4 only: the 8-wave selection must report them unsupported and leave out alone."""
    m = _m()
    prev = m.gemm_dw_impl(-1)
    try:
        m.gemm_dw_impl(impl)
        auto = m.gemm_dw_splits(T, M, N)
        if impl == 0 and M % 256:
            out = torch.full((M, N), 3.0, dtype=BF16, device="cuda")
            assert auto == 0 and not m.gemm_dw(torch.zeros(T, M, dtype=BF16, device="cuda"),
                                               torch.zeros(T, N, dtype=BF16, device="cuda"), out, True, 1)
            assert same_bits(out, torch.full_like(out, 3.0))
            return
        assert auto >= 1
        if (T // 64) % 2:
            # gemm_dw4 takes k-tiles in pairs: it declines (a half-height shape of this T is
            # unsupported outright) and the one split reported is the 8-wave loop's
            assert auto == 1 and m.gemm_dw_splits(T, M + 128, N) == 0
        c = dense_case(T, M, N)
        record(f"gemm_dw dense {(T, M, N)} impl {impl}: forced 1 split (default {auto})")
        ops = dev(c["dy"]), dev(c["x"])
        for accumulate in (False, True):
            run(m, c, ops, accumulate, 1, f"gemm_dw {(T, M, N)} impl {impl} accumulate {accumulate}")
    finally:
        m.gemm_dw_impl(prev)


@pytest.mark.parametrize("T,M,N,impls,split_counts", SPLIT)
def test_gemm_dw_any_split_exact(T, M, N, impls, split_counts):
    """Sparse dy (every partial bf16-exact, every k-step of every 128-column block occupied): the same
    bits RNE_bf16(base + exact) at every forced split count and at the default one, accumulate off
    and on."""
    m, c = _m(), sparse_case(T, M, N)
    ops = dev(c["dy"]), dev(c["x"])
    prev = m.gemm_dw_impl(-1)
    try:
        for impl in impls:
            m.gemm_dw_impl(impl)
            auto = m.gemm_dw_splits(T, M, N)
            assert 1 <= auto <= 16
            record(f"gemm_dw sparse {(T, M, N)} impl {impl}: forced splits {split_counts}, default {auto}")
            for splits in split_counts + (0,):
                for accumulate in (False, True):
                    run(m, c, ops, accumulate, splits,
                        f"gemm_dw {(T, M, N)} impl {impl} splits {splits or f'default {auto}'} accumulate {accumulate}")
    finally:
        m.gemm_dw_impl(prev)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("T,M,N,why", UNSUPPORTED)
def test_gemm_dw_unsupported_keeps_out(T, M, N, why, impl):
    """An unsupported shape reports 0 splits, gemm_dw returns False and a sentinel-filled out keeps its bits."""
    m = _m()
    prev = m.gemm_dw_impl(-1)
    try:
        m.gemm_dw_impl(impl)
        assert m.gemm_dw_splits(T, M, N) == 0, why
        sentinel = (torch.arange(M * N, dtype=torch.float32, device="cuda").reshape(M, N) % 251 - 125.5).to(BF16)
        for accumulate in (False, True):
            out = sentinel.clone()
            ok = m.gemm_dw(torch.ones(T, M, dtype=BF16, device="cuda"), torch.ones(T, N, dtype=BF16, device="cuda"),
                           out, accumulate)
            assert not ok, why
            assert same_bits(out, sentinel), why
    finally:
        m.gemm_dw_impl(prev)
