"""CPU self-checks of what test_gemm_nt_exact_gpu.py holds the forward GEMM to: the exactness bound
and the operand magnitudes of every table entry (most exact products need a bf16 rounding; the
one-rounding and two-rounding contracts differ in a useful share of the elements), the GELU cases'
argument range and ambiguity-band share, the float64 GELU and its derivative against PyTorch, the
mask-bit convention, the rounding and band classifier on hand-made values, the tables against the
host code's dispatch rules, and the comparison helpers on mutated references (a dropped k-slice, a
rounding too many or too few, a displaced bias-gradient partial row: each must fail and name the
right tile)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gemm_nt_exact_gpu as ng
from test_gemm_dw_exact_gpu import first_mismatch
from test_gemm_nt_exact_gpu import (BAND_FLOOR, DELTA, NT4, RING, TABLE, activation_expect, addend, as_bf16, build_case,
                                    classify, db_bound, gelu64, gelu_arg, gelu_grad64, keep_bits, linear_refs,
                                    nt4_tile_coords, on_ring, persistent_rows, pre_act, rne, rne_bf16, saved_grad,
                                    saved_refs, sid, stats_case, table_case)

F64 = torch.float64
BF16 = torch.bfloat16
NEEDS_ROUNDING_MIN = 0.5   # share of exact products that are not bf16-representable
CONTRACTS_DIFFER_MIN = 0.05  # share of elements where one rounding and two roundings differ (EPI 4, 5, 6)
BAND_MAX = 0.10            # share of activation outputs inside the ambiguity band
X_STD = (1.0, 2.5)         # standard deviation of the GELU argument


def record(line):
    print(f"[exact-cpu] {line}")


def share(mask):
    return float(mask.double().mean())


# ---------------------------------------------------------------------------------------------
# rounding, neighbours, band
# ---------------------------------------------------------------------------------------------
def test_rne_rounds_once_and_to_even():
    """rne() against hand-made values: ties to even, the spacing change at a power of two, signs and
    zero, and a value on which rounding through float32 first (twice) gives the other neighbour."""
    v = torch.tensor([257.0, 259.0, 258.0, -257.0, 1.0, 0.0, 255.5, 256.5, 2.0 ** -20 * 3, 1 + 2.0 ** -8,
                      1 + 2.0 ** -8 + 2.0 ** -30, 1 - 2.0 ** -10], dtype=F64)
    want = [256.0, 260.0, 258.0, -256.0, 1.0, 0.0, 256.0, 256.0, 2.0 ** -20 * 3, 1.0, 1 + 2.0 ** -7, 1.0]
    assert rne(v).tolist() == want
    twice = v.to(torch.float32).to(BF16).to(F64)  # float64 -> float32 ties 1 + 2^-8 + 2^-30 down to 1 + 2^-8
    assert twice[10] == 1.0 and rne(v)[10] == 1 + 2.0 ** -7
    # wherever float32 holds v exactly, PyTorch's own float32 -> bf16 conversion agrees
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 16, generator=g).to(F64) * torch.exp2(torch.randint(-30, 20, (1 << 16,), generator=g).to(F64))
    assert torch.equal(rne(x), x.to(torch.float32).to(BF16).to(F64))
    assert rne_bf16(torch.tensor([-0.0], dtype=F64)).view(torch.int16).item() == -32768  # a zero keeps its sign
    with pytest.raises(AssertionError):
        as_bf16(torch.tensor([257.0], dtype=F64))


def test_band_classifier_on_hand_made_values():
    """classify(): the neighbours of a value, a value exactly at a midpoint, just inside and just
    outside the band, the floor for small values, and representable values (never ambiguous)."""
    mid = 1.0 + 2.0 ** -8                       # between 1 and 1 + 2^-7
    inside, outside = mid * (1 + 0.9 * DELTA), mid * (1 + 1.2 * DELTA)
    small_mid = 2.0 ** -9 * (1 + 2.0 ** -8)     # |v| < floor: the band is DELTA * 2^-4 = 2^-18, wider than the spacing
    v = torch.tensor([mid, inside, outside, -outside, 1.0, 1.5, small_mid, 2.0 ** -9 * 1.25, 0.0, 3.0 - 2.0 ** -7],
                     dtype=F64)
    lo, hi, near, amb = classify(v)
    assert lo[:3].tolist() == [1.0] * 3 and hi[:3].tolist() == [1 + 2.0 ** -7] * 3
    assert near[:4].tolist() == [1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -7, -(1 + 2.0 ** -7)]   # the tie goes to even
    assert amb.tolist() == [True, True, False, False, False, False, True, False, False, True]
    assert lo[9] == 3.0 - 2.0 ** -6 and hi[9] == 3.0 and near[9] == 3.0   # a midpoint whose even neighbour is above
    assert bool((lo[[4, 5, 7, 8]] == hi[[4, 5, 7, 8]]).all())
    # at the floor: v = 2^-4 (1 + 2^-8): band = DELTA * |v|; just below the floor the band stops shrinking
    at = 2.0 ** -4 * (1 + 2.0 ** -8)
    w = torch.tensor([at * (1 + 0.99 * DELTA), at * (1 + 1.01 * DELTA + 2.0 ** -30),
                      0.5 * at + 0.99 * DELTA * BAND_FLOOR, 0.5 * at + 1.01 * DELTA * BAND_FLOOR], dtype=F64)
    assert classify(w)[3].tolist() == [True, False, True, False]
    # activation_expect: the nearest always passes; the other neighbour only inside the band; a
    # value two steps away or a NaN never
    got = torch.tensor([1 + 2.0 ** -7, 1.0, 1.0, 1 + 2.0 ** -6, float("nan")], dtype=BF16)
    vv = torch.tensor([mid, inside, outside, inside, inside], dtype=F64)
    want, other, n_amb = activation_expect(got, vv)
    assert (other, n_amb) == (2, 4)
    ok = want.view(torch.int16) == got.view(torch.int16)
    assert ok.tolist() == [True, True, False, False, False]
    assert want[2:].to(F64).tolist() == [1 + 2.0 ** -7] * 3


def test_float64_gelu_matches_pytorch():
    x = torch.linspace(-8, 8, 4001, dtype=F64, requires_grad=True)
    y = F.gelu(x, approximate="tanh")
    (g,) = torch.autograd.grad(y.sum(), x)
    xd = x.detach()
    assert float((gelu64(xd) - y.detach()).abs().max()) < 1e-14
    assert float((gelu_grad64(xd) - g).abs().max()) < 1e-14
    # the logistic form the kernels use (x * sigmoid(2u)) is the same function
    u = 0.7978845608028654 * (xd + 0.044715 * xd ** 3)
    assert float((xd * torch.sigmoid(2 * u) - gelu64(xd)).abs().max()) < 1e-14


def test_mask_bit_convention():
    """bit q of byte (m N + n) >> 3 keeps element n + q (n % 8 == 0): numpy's little-endian unpacking
    of the row-major byte stream."""
    M, N = 4, 24
    g = torch.Generator().manual_seed(5)
    mask = torch.randint(0, 256, (M * N // 8,), generator=g, dtype=torch.uint8)
    keep = keep_bits(mask, M, N)
    assert np.array_equal(keep.numpy(), np.unpackbits(mask.numpy(), bitorder="little").reshape(M, N).astype(np.float64))
    for m, n, q in ((0, 0, 0), (1, 8, 7), (3, 16, 3)):
        assert keep[m, n + q] == (int(mask[(m * N + n) >> 3]) >> q) & 1
    one = torch.zeros(M * N // 8, dtype=torch.uint8)
    one[(2 * N + 8) >> 3] = 1 << 5
    assert keep_bits(one, M, N).nonzero().tolist() == [[2, 13]]


# ---------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------
def test_tables_follow_the_dispatch_rules():
    """Every entry's mainloop by gemm_nt.hip's nt4_path (impl >= 1, K % 128 == 0, K >= 256) and
    gemm_nt_ok; each mainloop has its shortest K, a multi-tile-row shape and (4-wave) a half-width
    shape; the edges the table claims."""
    for (M, N, K), (impl, s, why) in TABLE.items():
        nt4 = impl >= 1 and K % 128 == 0 and K >= 256
        assert on_ring((M, N, K)) == (not nt4) and ((M, N, K) in RING) == (not nt4), why
        assert M % 256 == 0 and K % 64 == 0 and (N % 256 == 0 or (N % 256 == 128 and nt4)), why
    assert {k[2] for k in RING} >= {64, 128} and RING[(512, 512, 320)][0] == 1
    assert min(k[2] for k in NT4) == 256 and max(k[2] for k in NT4 if k[2] <= 1024) == 1024
    assert min(k[2] for k in NT4 if k[2] > 1024) == 1152       # K > 1024 launches the mirrored kernel
    assert any(k[0] > 256 for k in RING) and any(k[0] > 256 for k in NT4)
    assert sum(k[1] % 256 == 128 for k in NT4) >= 2
    assert any((k[0] // 256) * (k[1] // 256) % 8 for k in RING) and any((k[0] // 256) % 4 for k in NT4 if k[0] > 1024)


@pytest.mark.parametrize("shape", list(TABLE), ids=sid)
def test_operands_exact_and_rounding_contracts_distinguishable(shape):
    """The < 2^24 bound (build_case asserts it), operands and addends bf16-representable, at least
    half of the exact products in need of a rounding, the two contracts of EPI 4 / 5 / 6 different in
    at least 5 % of the elements, and EPI 8's per-column bound."""
    c = table_case(shape)
    u = c["u"]
    for t in (c["a"], c["b"] * u, c["bias"] * u, addend(c) * u, c["gbias"], pre_act(c), saved_grad(c), c["base"] * u):
        as_bf16(t)
    assert float(c["p"].abs().max()) + ng.BIAS_MAX + ng.ADD_STEP * ng.ADD_MAX < ng.LIM
    assert not bool(torch.signbit(c["p"][c["p"] == 0]).any())   # the accumulators start at +0: no -0 product sums
    needs = share(rne(c["p"]) != c["p"])
    ring, nt4 = linear_refs(c, True), linear_refs(c, False)
    differ = {e: share(ring[e] != nt4[e]) for e in (4, 5, 6)}
    record(f"{sid(shape)}: {needs:.1%} of the products need rounding; one vs two roundings differ in "
           + ", ".join(f"EPI {e} {v:.1%}" for e, v in differ.items()))
    assert needs >= NEEDS_ROUNDING_MIN
    assert min(differ.values()) >= CONTRACTS_DIFFER_MIN
    assert torch.equal(ring[0], nt4[0]) and torch.equal(ring[1], nt4[1])
    for refs in (ring, nt4):
        for e, v in refs.items():
            as_bf16(v * u)
    # the mask matters: EPI 6 differs from EPI 4 and from EPI 0
    assert share(nt4[6] != nt4[4]) > 0.2 and share(nt4[6] != nt4[0]) > 0.2
    if not on_ring(shape):
        want = saved_refs(c)  # asserts sum_m |d| * 4 < 2^24 per column
        assert share(want["dx"] != c["p"] * saved_grad(c)) > 0.1 and share(want["db"] != want["db_acc"]) > 0.5


@pytest.mark.parametrize("shape", list(TABLE), ids=sid)
def test_gelu_cases_stay_in_range_and_mostly_outside_the_band(shape):
    """Per GELU-family output of each table entry: max |x| <= 8, the argument's standard deviation in
    [1, 2.5], at most 10 % of the reference values inside the ambiguity band; and the two mainloops'
    references (argument rounded to bf16 or not) differ visibly."""
    c = table_case(shape)
    ring = on_ring(shape)
    outs = {}
    x2 = gelu_arg(c, ring) + c["gbias"]
    outs["EPI 2 Y"] = (x2, gelu64(x2))
    x3 = pre_act(c) + c["gbias"]
    # pre + bias is exact in fp32: a multiple of 2^-6 below 2^18 steps
    assert float((x3 * 64).abs().max()) <= ng.PRE_MAX + ng.GB_MAX and torch.equal((x3 * 64).round(), x3 * 64)
    outs["EPI 3 dx"] = (x3, gelu_arg(c, ring) * gelu_grad64(x3))
    if not ring:
        outs["EPI 7 C"] = (x2, gelu_grad64(x2))
    for name, (x, v) in outs.items():
        amb = share(classify(v)[3])
        record(f"{sid(shape)} {name}: max |x| {float(x.abs().max()):.3f}, std {float(x.std()):.3f}, "
               f"ambiguity band {amb:.2%}")
        assert float(x.abs().max()) <= ng.X_LIMIT
        assert X_STD[0] <= float(x.std()) <= X_STD[1]
        assert amb <= BAND_MAX
    # the other mainloop's argument gives other bits in a useful share of the outputs
    xo = gelu_arg(c, not ring) + c["gbias"]
    assert share(rne(gelu64(xo)) != rne(gelu64(x2))) >= CONTRACTS_DIFFER_MIN
    assert share(rne(gelu_arg(c, not ring) * gelu_grad64(x3)) != rne(outs["EPI 3 dx"][1])) >= CONTRACTS_DIFFER_MIN


@pytest.mark.parametrize("shape", [s for s in TABLE if not (on_ring(s) and s[1] % 256)], ids=sid)
def test_stats_cases_are_exact_and_offset(shape):
    """EPI 9 inputs: integers within the bound (stats_case asserts it), and channels whose mean
    dwarfs their spread."""
    c = stats_case(*shape)
    out = c["c"]
    assert torch.equal(out, out.round()) and bool((c["a"][:, 0] == ng.STATS_A0).all())
    ratio = out.mean(0).abs() / out.std(0)
    assert float(ratio.max()) > 3.0 and float(ratio.min()) < 0.5


def test_persistent_case_reaches_two_tiles_with_a_halfn_change():
    """The persistent-grid case at 256 CUs: 8448 rows, 297 tiles; coords() is a bijection onto the
    tile grid for its and the table's grids; workgroups whose two tiles differ in halfn exist; the
    case's bounds hold (EPI 8's column sums included)."""
    assert persistent_rows(256) == 8448
    for cus in (256, 304, 64, 8):
        M = persistent_rows(cus)
        assert (M // 256) * 9 > cus and (M // 256) * 9 % cus != 0
    N, K = ng.PERSISTENT_NK
    for tiles_m, tiles_n in [(33, 9), (5, 1), (3, 3), (1, 2), (13, 197)]:
        seen = {nt4_tile_coords(v, tiles_m, tiles_n) for v in range(tiles_m * tiles_n)}
        assert seen == {(i, j) for i in range(tiles_m) for j in range(tiles_n)}
    half = [(nt4_tile_coords(v, 33, 9)[1] == 8, nt4_tile_coords(v + 256, 33, 9)[1] == 8)
            for v in range(297 - 256)]   # (halfn of the first tile, of the second) per two-tile workgroup
    assert any(a != b for a, b in half) and any(a == b for a, b in half)
    c = build_case(8448, N, K, ng.PERSISTENT_S, ng.PERSISTENT_B_MAG)
    needs = share(rne(c["p"]) != c["p"])
    want = saved_refs(c)
    record(f"persistent 8448x{N}x{K}: {needs:.1%} of the products need rounding; EPI 8 column bound at "
           f"{want['worst'] / ng.LIM:.3f} of 2^24")
    assert needs >= NEEDS_ROUNDING_MIN


# ---------------------------------------------------------------------------------------------
# the comparison helpers on mutated references
# ---------------------------------------------------------------------------------------------
MUT = (512, 512, 320)  # 2 x 2 tiles


def test_mismatch_names_a_flipped_bit():
    c = table_case(MUT)
    want = as_bf16(linear_refs(c, True)[1] * c["u"])
    assert first_mismatch(want.clone(), want) is None
    got = want.clone()
    got.view(torch.int16)[300, 257] ^= 1
    msg = first_mismatch(got, want)
    assert msg.startswith("first mismatch at tile (1, 1) row 44 column 1 (m 300, n 257)") and "(1 of 262144" in msg, msg


def test_mismatch_names_a_dropped_k_tile():
    """One 64-wide k-slice missing from the products of tile (1, 0) only: the helper fails and its
    first coordinate lies in that tile; nearly every element of the tile changes."""
    c = table_case(MUT)
    p = c["p"].clone()
    p[256:, :256] -= c["a"][256:, 128:192] @ c["b"][:256, 128:192].t()
    got, want = as_bf16(rne(p) * c["u"]), as_bf16(rne(c["p"]) * c["u"])
    msg = first_mismatch(got, want)
    assert msg is not None and msg.startswith("first mismatch at tile (1, 0) row 0 column"), msg
    assert share(got[256:, :256] != want[256:, :256]) > 0.9 and torch.equal(got[:256], want[:256])
    # a doubled 32-wide k-step of the ring likewise
    p = c["p"].clone()
    p[:256, 256:] += c["a"][:256, 32:64] @ c["b"][256:, 32:64].t()
    msg = first_mismatch(as_bf16(rne(p) * c["u"]), want)
    assert msg is not None and msg.startswith("first mismatch at tile (0, 1) row 0 column"), msg


def test_mismatch_tells_one_rounding_from_two():
    """The ring's reference against the 4-wave loop's for EPI 4, 5, 6 (a second rounding where one is
    specified, and the reverse), and a bias added after the rounding instead of before it."""
    c = table_case(MUT)
    ring, nt4 = linear_refs(c, True), linear_refs(c, False)
    for e in (4, 5, 6):
        for got, want in ((ring[e], nt4[e]), (nt4[e], ring[e])):
            msg = first_mismatch(as_bf16(got * c["u"]), as_bf16(want * c["u"]))
            assert msg is not None and msg.startswith("first mismatch at tile (0, 0) row 0 column"), (e, msg)
    late_bias = rne(rne(c["p"]) + c["bias"])
    assert share(late_bias != ring[1]) >= CONTRACTS_DIFFER_MIN
    assert first_mismatch(as_bf16(late_bias * c["u"]), as_bf16(ring[1] * c["u"])) is not None
    # the activation rule: an output computed from the other mainloop's argument is refused
    x = gelu_arg(c, True) + c["gbias"]
    other = rne_bf16(gelu64(gelu_arg(c, False) + c["gbias"]))
    want, _, _ = activation_expect(other, gelu64(x))
    assert first_mismatch(other, want) is not None
    mine = rne_bf16(gelu64(x))
    want, non_nearest, _ = activation_expect(mine, gelu64(x))
    assert first_mismatch(mine, want) is None and non_nearest == 0


def test_mismatch_names_a_displaced_partial_row():
    """EPI 8's bias gradient from its partial rows [2 tiles_m][N] (slot 2 tm + wm, 128 rows each).
    The partial of (tm 1, wm 0) written to the neighbouring slot in tile column 1 only — where it
    replaces that slot's own row, its own slot left at zero — changes db there and nowhere else; so
    does a partial row counted twice.  The EPI 3 bound notices the same displacement."""
    shape = (512, 256, 384)
    c = table_case(shape)
    M, N, u = c["M"], c["N"], c["u"]
    d = c["p"] * saved_grad(c)
    part = d.view(M // 128, 128, N).sum(1)           # slot 2 tm + wm holds rows 256 tm + 128 wm ...
    want = saved_refs(c)
    assert torch.equal(rne(part.sum(0)), want["db"])
    c2 = table_case(MUT)
    d2 = c2["p"] * saved_grad(c2)
    part2 = d2.view(4, 128, 512).sum(1)
    moved = part2.clone()
    moved[3, 256:] = part2[2, 256:]
    moved[2, 256:] = 0
    db, ref = as_bf16(rne(moved.sum(0)) * c2["u"]).view(1, -1), as_bf16(rne(part2.sum(0)) * c2["u"]).view(1, -1)
    msg = first_mismatch(db, ref)
    assert msg is not None and msg.startswith("first mismatch at tile (0, 1) row 0 column 0 (m 0, n 256)"), msg
    twice = part2.clone()
    twice[1, :256] *= 2
    msg = first_mismatch(as_bf16(rne(twice.sum(0)) * c2["u"]).view(1, -1), ref)
    assert msg is not None and msg.startswith("first mismatch at tile (0, 0) row 0 column"), msg
    # EPI 3 (not bit-exact): the same displacement against the per-column bound
    x = pre_act(c2) + c2["gbias"]
    d3 = gelu_arg(c2, False) * gelu_grad64(x)
    part3 = d3.view(4, 128, 512).sum(1)
    moved3 = part3.clone()
    moved3[3, 256:] = part3[2, 256:]
    moved3[2, 256:] = 0
    bound = db_bound(d3.sum(0), d3.abs().sum(0), 512)
    ratio = (rne(moved3.sum(0)) - d3.sum(0)).abs() / bound
    assert float(ratio[:256].max()) <= 1.0 and float(ratio[256:].median()) > 10.0
    # and the bound is of the size the text says: at most 2^-8 |ref| plus 2^-14 + M 2^-24 of the absolute sum
    assert float((bound / (d3.abs().sum(0) * (DELTA + 512 * 2.0 ** -24) + 2.0 ** -8 * d3.sum(0).abs())).max()) <= 1.0
