"""Bit-exact checks of the grouped weight-gradient GEMM (gemm_dw4.hip gemm_dw4_grouped, bound as
gemm_dw_grouped): several problems out_i[M_i][N_i] (+)= dy_i^T x_i in one launch, each 256 x 256
tile over its whole token axis.

Method of test_gemm_dw_exact_gpu.py: integer-valued bf16 operands with T * max|dy| * max|x| +
max|base| < 2^24, so every fp32 sum the kernel can form is exact, and the expected output is the
float64 product (plus base) rounded once to bf16.  Workgroup-to-tile mapping, the problem table and
k offsets are all covered this way: a tile computed from another problem's operands, a k-tile
dropped or doubled, or a tile nobody wrote changes bits.

On real-valued data the grouped result is RNE_bf16(base + fp32 sum): bit-identical to the
single-problem kernel with one split, and (one rounding against two) no further from the float64
product than the split-K path; that margin is measured in the test, not a constant.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
LIM = 1 << 24
V_MAX, BASE_MAX = 4, 8


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _bits(t):
    return t.contiguous().view(torch.int16)


def first_mismatch(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    ne = _bits(got) != _bits(want)
    count = int(ne.sum())
    if count == 0:
        return None
    m, n = divmod(int(ne.reshape(-1).nonzero()[0]), got.shape[1])
    return f"first mismatch at tile ({m // 256}, {n // 256}) row {m % 256} column {n % 256}: got " \
           f"{float(got[m, n])!r}, expected {float(want[m, n])!r} ({count} of {got.numel()} elements differ)"


def ints(shape, amax, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amax, amax + 1, shape, generator=g, dtype=torch.int8)


@functools.lru_cache(maxsize=None)
def case(T, M, N, seed):
    """(dy, x, base int8; float64 dy^T x) of one problem — computed once, never modified."""
    assert T * V_MAX * V_MAX + BASE_MAX < LIM
    dy, x, base = ints((T, M), V_MAX, seed), ints((T, N), V_MAX, seed + 1), ints((M, N), BASE_MAX, seed + 2)
    return dy, x, base, dy.to(F64).t() @ x.to(F64)


def expected(ref, base, accumulate):
    t = ref + base.to(F64) if accumulate else ref
    assert float(t.abs().max()) < LIM
    return t.to(torch.float32).to(BF16)


def strided(t, pad_before, pad_after, dev):
    """t as a column slice of a wider row-major buffer (an arena-slice view: row stride > row)."""
    buf = torch.full((t.shape[0], pad_before + t.shape[1] + pad_after), 77.0, dtype=BF16, device=dev)
    v = buf[:, pad_before:pad_before + t.shape[1]]
    v.copy_(t.to(BF16))
    return buf, v


def run_group(probs, accs, pads=None):
    """probs: [(T, M, N)], accs: [bool], pads: None or per problem (dy, x, out) column paddings
    (before, after) or None.  Runs one gemm_dw_grouped call and checks every output bit for bit, and
    that the padding around a strided output is untouched."""
    dev = torch.device("cuda", 0)
    dys, xs, outs, wants, guards = [], [], [], [], []
    for i, (T, M, N) in enumerate(probs):
        dy, x, base, ref = case(T, M, N, 1000 * i + (T + 3 * M + 7 * N) % 997)
        pd = pads[i] if pads else (None, None, None)
        dys.append(strided(dy, *pd[0], dev)[1] if pd[0] else dy.to(dev).to(BF16))
        xs.append(strided(x, *pd[1], dev)[1] if pd[1] else x.to(dev).to(BF16))
        if pd[2]:
            buf, o = strided(base, *pd[2], dev)
            guards.append((buf, pd[2], N))
        else:
            o = base.to(dev).to(BF16)
        outs.append(o)
        wants.append(expected(ref, base, accs[i]))
    assert _m().gemm_dw_grouped(dys, xs, outs, list(accs)) is True
    torch.cuda.synchronize()
    for i, (o, want) in enumerate(zip(outs, wants)):
        msg = first_mismatch(o.cpu(), want)
        assert msg is None, f"problem {i} {probs[i]} accumulate={accs[i]}: {msg}"
    for buf, (b, a), N in guards:
        assert bool((buf[:, :b] == 77.0).all()) and bool((buf[:, b + N:] == 77.0).all()), "padding overwritten"


def test_one_problem_shortest_pipeline():
    run_group([(256, 256, 256)], [False])
    run_group([(256, 256, 256)], [True])


def test_two_problems_different_T_half_height_row():
    run_group([(256, 256, 256), (640, 384, 512)], [True, True])


def test_mixed_accumulate():
    run_group([(256, 256, 256), (640, 384, 512), (384, 128, 256)], [False, True, False])


def test_strided_operands_and_outputs():
    # row strides larger than the rows; output 2: a start that is not 8-byte aligned (element stores)
    pads = [((8, 8), (16, 0), (64, 64)), (None, (0, 8), (0, 4)), ((0, 24), None, (3, 5))]
    run_group([(256, 256, 256), (640, 384, 512), (384, 256, 256)], [True, False, True], pads)


def test_two_rounds_in_one_launch():
    # 20 x 16 = 320 tiles: past 256 workgroups (a full round by XCD blocks, then a partial round)
    run_group([(256, 1024, 1024)] * 20, [i % 2 == 0 for i in range(20)])


def test_more_problems_than_the_table_holds():
    # 34 problems: the 32-entry table, then a second launch with 2
    run_group([(256, 256, 256)] * 33 + [(256, 128, 512)], [True] * 34)


def test_problem_after_a_tile_count_not_a_multiple_of_32():
    # 6 tiles (with a half-height row), then 16 x 4 = 64 tiles starting at tile 6 of the XCD blocks,
    # then a 5-column problem (a narrower last strip)
    run_group([(256, 640, 512), (256, 4096, 1024), (256, 512, 1280)], [True, True, False])


def test_long_k_beside_short():
    run_group([(65536, 256, 256), (256, 256, 256)], [True, True])


@pytest.mark.parametrize("bad", [(1000, 256, 256), (256, 256, 128), (256, 192, 256), (128, 256, 256), (192, 256, 256)])
def test_out_of_contract_problem_launches_nothing(bad):
    dev = torch.device("cuda", 0)
    probs = [(256, 256, 256), bad, (256, 256, 256)]
    dys = [torch.ones(T, M, dtype=BF16, device=dev) for T, M, N in probs]
    xs = [torch.ones(T, N, dtype=BF16, device=dev) for T, M, N in probs]
    outs = [torch.full((M, N), 5.0, dtype=BF16, device=dev) for T, M, N in probs]
    assert _m().gemm_dw_grouped(dys, xs, outs, [True] * 3) is False
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 5.0).all()), "an output was written although the call declined"


def _real(shape, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32).to(BF16)


def test_real_data_equals_single_problem_one_split():
    dev = torch.device("cuda", 0)
    m = _m()
    probs = [(1024, 384, 512), (2048, 256, 256)]
    dys = [_real((T, M), 10 + i, dev) for i, (T, M, N) in enumerate(probs)]
    xs = [_real((T, N), 20 + i, dev) for i, (T, M, N) in enumerate(probs)]
    bases = [_real((M, N), 30 + i, dev) for i, (T, M, N) in enumerate(probs)]
    grouped = [b.clone() for b in bases]
    assert m.gemm_dw_grouped(dys, xs, grouped, [True, True]) is True
    prev = m.gemm_dw_impl(1)
    try:
        for dy, x, b, got in zip(dys, xs, bases, grouped):
            single = b.clone()
            assert m.gemm_dw(dy, x, single, True, 1) is True
            msg = first_mismatch(got.cpu(), single.cpu())
            assert msg is None, msg
    finally:
        m.gemm_dw_impl(prev)


def test_real_data_error_not_above_split_k():
    """RMS error against the float64 product: grouped (one rounding) <= split-K (partials rounded to
    bf16, then the fold's rounding) measured here on the same data."""
    dev = torch.device("cuda", 0)
    m = _m()
    T, M, N = 4096, 256, 512
    dy, x = _real((T, M), 1, dev), _real((T, N), 2, dev)
    ref = dy.cpu().to(F64).t() @ x.cpu().to(F64)
    got = torch.empty(M, N, dtype=BF16, device=dev)
    assert m.gemm_dw_grouped([dy], [x], [got], [False]) is True
    split = torch.empty(M, N, dtype=BF16, device=dev)
    prev = m.gemm_dw_impl(1)
    try:
        assert m.gemm_dw(dy, x, split, False, 8) is True
    finally:
        m.gemm_dw_impl(prev)
    rms = lambda t: float((t.cpu().to(F64) - ref).pow(2).mean().sqrt())
    e_grouped, e_split = rms(got), rms(split)
    print(f"rms error vs float64: grouped {e_grouped:.6g}, split-K(8) {e_split:.6g}")
    assert e_grouped <= e_split
