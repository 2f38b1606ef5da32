"""Bit-exact checks of the forward-layout GEMM C[M][N] = A[M][K] B[N][K]^T and its ten epilogues
(gemm_nt.hip: the 8-wave ring; gemm_nt4.hip: the 4-wave persistent mainloop).

Method.  A holds integers in [-15, 15]; B holds integers of magnitude 8 .. 15 (a table entry may
narrow that) times 2^-s, s per shape: every operand is a bf16 value "integer x 2^-s" (dyadic).  Every
product and every fp32 partial sum a kernel can form, in any order, is then a multiple of 2^-s whose
integer part stays below 2^24, so the fp32 accumulators are exact whatever the tile, wave, MFMA or
k order.  The bound, in units of 2^-s, is asserted per case while it is built:

    K * max|a| * max|b| + max|bias| + max|addend| < 2^24          (g = s)

The expected value is the float64 matmul on the CPU pushed through the epilogue's rounding contract
(never through a kernel); comparisons are on bit patterns; a mismatch is reported at its first
element as (tile row, tile column, row and column in the 256 x 256 tile) with the count
(first_mismatch of test_gemm_dw_exact_gpu.py).  Magnitudes up to 15 make most exact products carry
more than 8 significant bits, so one rounding and two roundings give different bits in a large share
of the elements (test_gemm_nt_exact_cpu.py asserts both shares for every table entry).

The bindings only ever pass dense strides (lda = ldb = K, ldc = ldy = N); nothing else is tested.

Rounding contracts, read from the epilogues.  P is the exact product, f() the bf16 -> fp32
conversion, RNE round-to-nearest-even to bf16, r the addend, keep the addend's mask bit.

    EPI  8-wave ring (gemm_nt_impl(0), K < 256 or K % 128 != 0)   4-wave (gemm_nt4)
    0    RNE(P)                                                   same
    1    RNE(P + bias)                                            same
    4    RNE(f(RNE(P)) + r)                                       RNE(P + r)
    5    RNE(f(RNE(P + bias)) + r)                                RNE((P + bias) + r), exact in fp32
    6    RNE(f(RNE(P)) + keep r)                                  RNE(P + keep r)
    2    C = RNE(P), Y ~ gelu(f(C) + bias)                        C = RNE(P), Y ~ gelu(P + bias)
    3    dx ~ f(RNE(P)) gelu'(pre + bias)                         dx ~ P gelu'(pre + bias)
    7    declined (code -4)                                       C ~ gelu'(P + bias), Y ~ gelu(P + bias)
    8    declined (code -4)                                       dx = RNE(P Y); bias-gradient partials exact
    9    C = RNE(P); sum and centred sum of squares of the        same per 128-row group (tile, wm)
         bf16 outputs per 256-row group

EPI 6: bit q of mask byte (m N + n) >> 3 (n % 8 == 0) keeps element n + q of row m.
EPI 3 / 8 write fp32 column partials of the unrounded dx, one row per (tile row, wave) on the ring
(slot 8 tm + w, 32 rows each) and per (tile row, wm) on the 4-wave loop (slot 2 tm + wm, 128 rows);
reduce.hip colsum adds the rows in fp32 and converts once: db = RNE(sum), and with db_out= (ColOut.acc)
db = RNE(f(base) + sum) — the bf16 base joins the fp32 sum before the one rounding.

Bit-exact: everything of EPI 0, 1, 4, 5, 6, C of EPI 2, the group sums of EPI 9 (the bf16 outputs
are integers; the shifted sums and Chan merges add integers below 2^24), and EPI 8 whole: the saved
derivative Y is a multiple of 1/4 in [-0.25, 1.25], so P Y, the partials and the column sum are
exact (asserted per column: sum_m |d| * 4 * 2^s < 2^24).  The centred sum of squares of EPI 9 keeps
the project's tolerance for per-group partials (check_tile_stats of test_conv_exact_gpu.py).

The activation outputs (Y of EPI 2 / 7, C of EPI 7, dx of EPI 3) go through gelu_sig* (common.h):
fp32 with one hardware exp2 and one rcp, not bit-reproducible from float64.  The reference v is the
float64 tanh-GELU (or its derivative, times the exact argument above).  Every element must be one
of the two bf16 neighbours of v, and must equal RNE(v) bit for bit unless v lies within
DELTA * max(|v|, 2^-4) of the bf16 rounding midpoint, DELTA = 2^-14: about ten fp32 operations with
1-ulp exp2 / rcp plus the exponent's amplification |z| ln 2 2^-24, |z| <= 71 at |x| <= 8, stay under
2^-16 relative (4x margin); the floor covers gelu' near its zero crossing, where the error is
absolute.  db of EPI 3 is compared with the float64 column sum of the unrounded reference, per
column within ulp_bf16(ref) / 2 + (DELTA + M 2^-24) sum_m |d_ref|.

Guards.  gemm_nt(out=) runs into a NaN-filled out; before every other call a NaN block of each
output's size is filled and released (the caching allocator tends to hand it to the next at::empty
of that size), and no identical case runs twice in a row.  test_gemm_nt_exact_cpu.py validates the
builders, tables, preconditions and comparison helpers of this file.
"""
import functools

import pytest
import torch

from test_conv_exact_gpu import check_tile_stats
from test_gemm_dw_exact_gpu import check_bits, same_bits

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
LIM = 1 << 24
DELTA = 2.0 ** -14        # relative half-width of the ambiguity band around a rounding midpoint
BAND_FLOOR = 2.0 ** -4    # the band is DELTA * max(|v|, BAND_FLOOR)
X_LIMIT = 8.0             # max |x| of every GELU argument (beyond it rcp reaches denormals)
A_MAX = 15                # A: integers in [-A_MAX, A_MAX]
B_MAG = (8, 15)           # B: integer magnitudes in [lo, hi] with a random sign, times 2^-s
BIAS_MAX = 255            # bias of the integer epilogues (units of 2^-s)
ADD_STEP, ADD_MAX = 8, 255  # addend r = ADD_STEP * j, |j| <= ADD_MAX (units of 2^-s)
GB_STEP, GB_MAX = 2.0 ** -6, 96    # GELU bias = GB_STEP * j, |j| <= GB_MAX: [-1.5, 1.5]
PRE_MAX = 128                      # saved pre-activation of EPI 3 = GB_STEP * j, |j| <= PRE_MAX: [-2, 2]
DB_BASE_MAX = 255                  # db_out= base of EPI 8 (units of 2^-s)
# saved gelu' of EPI 8: multiples of 1/4 in [-0.25, 1.25], half of them 0 (gelu' of a negative argument)
SAVED_GRAD = (0.0,) * 8 + (1.0,) * 3 + (-0.25, 0.25, 0.5, 0.75, 1.25)
STATS_A_MAX, STATS_A0 = 3, 256     # EPI 9: A in [-3, 3] with column 0 = 256, so |mean| >> std in some channels

# (M, N, K): (impl, s, why).  s scales B so that x = P + bias has a standard deviation in [1, 2.5].
RING = {
    (256, 256, 64): (0, 10, "nk = 2 k-steps of 32, below the ring's 5 stages"),
    (256, 256, 128): (0, 10, "nk = 4, one short of the stages"),
    (768, 256, 192): (0, 11, "nk = 6; 3 tiles: the XCD remap has a remainder"),
    (512, 512, 320): (1, 11, "left at impl 1: K % 128 != 0 must still take the ring; 2 x 2 tiles"),
    (256, 512, 1024): (0, 12, "32 k-steps: the ring wraps six times"),
}
NT4 = {
    (256, 256, 256): (1, 11, "nk = 4 k-tiles of 64: the shortest legal pipeline"),
    (512, 256, 384): (1, 11, "nk = 6; two tile rows"),
    (256, 384, 256): (1, 11, "half-width last tile column: wn = 1 waves store nothing"),
    (768, 640, 512): (1, 12, "half-width column with 3 tile rows; 9 tiles: remap remainder"),
    (1280, 256, 256): (1, 11, "5 tile rows: the last group of group_m = 4 is short"),
    (256, 256, 1024): (1, 12, "the last K on the B-stationary (non-mirrored) launch"),
    (256, 512, 1152): (1, 12, "the first mirrored (MIR) launch"),
    (512, 256, 2048): (1, 13, "mirrored, 32 k-tiles, two tile rows"),
}
TABLE = {**RING, **NT4}
PERSISTENT_NK = (2176, 256)  # N (8.5 tile columns), K of the persistent-grid case; M from the CU count
PERSISTENT_S = 11
PERSISTENT_B_MAG = (4, 11)   # keeps sum_m |P Y| * 4 below 2^24 over 8448 rows


def sid(shape):
    return "x".join(map(str, shape))


def on_ring(shape):
    M, N, K = shape
    return TABLE[shape][0] == 0 or K < 256 or K % 128 != 0


def persistent_rows(cus):
    """M of the persistent-grid case: 9 tile columns (the last half wide) and enough tile rows that
    tiles > CUs and tiles % CUs != 0 — 8448 rows = 33 x 9 = 297 tiles on 256 CUs."""
    tiles_m = -(-(cus + 40) // 9)
    while tiles_m * 9 <= cus or (tiles_m * 9) % cus == 0:
        tiles_m += 1
    return 256 * tiles_m


def nt4_tile_coords(v, tiles_m, tiles_n, group_m=4):
    """gemm_nt4.hip coords(): virtual tile id -> (tile row, tile column)."""
    nwg = tiles_m * tiles_n
    xcd, slot, q, r = v & 7, v >> 3, nwg >> 3, nwg & 7
    i = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot
    per_group = group_m * tiles_n
    g = i // per_group
    first_m = g * group_m
    gsz, rem = min(tiles_m - first_m, group_m), i - g * per_group
    return first_m + rem % gsz, rem // gsz


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


# ---------------------------------------------------------------------------------------------
# bf16 rounding, neighbours and the ambiguity band of float64 values (CPU)
# ---------------------------------------------------------------------------------------------
def _quantum(v):
    """The bf16 spacing at each float64 v (normal range): 2^(e - 8) for |v| in [2^(e-1), 2^e)."""
    _, e = torch.frexp(v)
    return ((e.to(torch.int64) - 8 + 1023) << 52).view(F64)  # 2^(e - 8), built from its exponent field


def as_bf16(t):
    """A float64 tensor of bf16-representable values as bf16 (both conversions exact)."""
    out = t.to(torch.float32).to(BF16)
    assert torch.equal(out.to(F64), t), "not bf16-representable"
    return out


def rne(v):
    """float64 -> the nearest bf16 value (ties to even) in ONE rounding, returned as float64; the sign
    of a zero is kept (EPI 8 stores the IEEE product -|P| * 0 = -0)."""
    q = _quantum(v)
    return torch.round(v / q) * q   # torch.round: half to even; v / q and * q are exact


def rne_bf16(v):
    return as_bf16(rne(v))


def classify(v, delta=DELTA, floor=BAND_FLOOR, band=None):
    """(lo, hi, near, ambiguous) of float64 v: its two bf16 neighbours (equal where v is
    representable), RNE(v), and whether v lies within delta * max(|v|, floor) of the midpoint of
    lo and hi (never where v is representable: the next midpoints are half a spacing away).
    band (optional): a float64 tensor of absolute half-widths per element, used instead of
    delta * max(|v|, floor)."""
    q = _quantum(v)
    lo, hi = torch.floor(v / q) * q, torch.ceil(v / q) * q
    near = torch.round(v / q) * q
    width = delta * v.abs().clamp_min(floor) if band is None else band
    amb = (lo != hi) & ((v - (lo + hi) * 0.5).abs() <= width)
    return lo, hi, near, amb


def activation_expect(got, v):
    """(want, non_nearest, ambiguous): want = got where got is acceptable for the float64 value v,
    RNE(v) elsewhere — so first_mismatch(got, want) names the first unacceptable element."""
    lo, hi, near, amb = classify(v)
    lo, hi, near = as_bf16(lo), as_bf16(hi), as_bf16(near)
    gb = got.view(torch.int16)
    is_near = gb == near.view(torch.int16)
    other = amb & ((gb == lo.view(torch.int16)) | (gb == hi.view(torch.int16))) & ~is_near
    want = torch.where(is_near | other, got, near)
    return want, int(other.sum()), int(amb.sum())


def check_activation(got, v, what):
    got = got.cpu()
    assert got.dtype == BF16 and got.shape == v.shape, (what, got.dtype, got.shape)
    want, other, amb = activation_expect(got, v)
    record(f"{what}: non-nearest neighbour in {other} of {v.numel()} = {other / v.numel():.4%} "
           f"(ambiguity band holds {amb / v.numel():.3%})")
    check_bits(got, want, what)


def gelu64(x):
    """tanh-GELU in float64."""
    u = 0.7978845608028654 * (x + 0.044715 * x ** 3)
    return 0.5 * x * (1.0 + torch.tanh(u))


def gelu_grad64(x):
    u = 0.7978845608028654 * (x + 0.044715 * x ** 3)
    t = torch.tanh(u)
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * x * x)


def keep_bits(mask, M, N):
    """EPI 6: bit q of byte i keeps element 8 i + q of the row-major [M, N] addend."""
    bits = (mask.to(torch.int32).view(-1, 1) >> torch.arange(8, dtype=torch.int32)) & 1
    return bits.reshape(M, N).to(F64)


def db_bound(ref_sum, abs_sum, M):
    """EPI 3: per-column bound of |db - float64 column sum|."""
    return 0.5 * _quantum(ref_sum) + (DELTA + M * 2.0 ** -24) * abs_sum


# ---------------------------------------------------------------------------------------------
# cases: inputs and float64 references (CPU, shared, never modified)
# ---------------------------------------------------------------------------------------------
def ints(shape, amax, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amax, amax + 1, shape, generator=g).to(F64)


def magnitudes(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    sign = 2 * torch.randint(0, 2, shape, generator=g) - 1
    return (sign * torch.randint(lo, hi + 1, shape, generator=g)).to(F64)


def build_case(M, N, K, s, b_mag=B_MAG):
    """Operands (in units of 2^-s: integers) and the exact product of one shape, on the CPU; `u` =
    2^-s turns the integer units into values.  The [M, N] inputs are kept in narrow types; use
    addend(), pre_act(), saved_grad() and keep_bits() for their float64 values."""
    seed = (M * 7 + N * 3 + K * 31 + s) % (1 << 31)
    a, b = ints((M, K), A_MAX, seed), magnitudes((N, K), b_mag[0], b_mag[1], seed + 1)
    bias = ints((N,), BIAS_MAX, seed + 2)
    r = ints((M, N), ADD_MAX, seed + 3).to(torch.int16)
    g = torch.Generator().manual_seed(seed + 4)
    mask = torch.randint(0, 256, (M * N // 8,), generator=g, dtype=torch.uint8)
    gbias = GB_STEP * ints((N,), GB_MAX, seed + 5)                 # values, multiples of 2^-6 >= 2^-s
    pre = ints((M, N), PRE_MAX, seed + 6).to(torch.int16)
    saved = torch.tensor(SAVED_GRAD, dtype=torch.float32)[torch.randint(0, len(SAVED_GRAD), (M, N), generator=g)]
    base = ints((N,), DB_BASE_MAX, seed + 7)
    u = 2.0 ** -s
    assert s >= 6 and GB_STEP / u == round(GB_STEP / u)            # the GELU bias is a multiple of 2^-s
    # every fp32 sum is an integer (units of 2^-s) below 2^24
    amax, bmax = float(a.abs().max()), float(b.abs().max())
    assert amax <= A_MAX and b_mag[0] <= float(b.abs().min()) and bmax <= b_mag[1]
    assert K * amax * bmax + BIAS_MAX + ADD_STEP * ADD_MAX < LIM
    assert K * amax * bmax + GB_MAX * GB_STEP / u < LIM
    p = a @ b.t() + 0.0    # exact: integers below 2^24 < 2^53; + 0.0: a sum of -0 products is +0 in the kernels
    assert float(p.abs().max()) + BIAS_MAX + ADD_STEP * ADD_MAX < LIM
    return dict(M=M, N=N, K=K, s=s, u=u, a=a, b=b, p=p, bias=bias, r=r, mask=mask, gbias=gbias, pre=pre,
                saved=saved, base=base)


case = functools.lru_cache(maxsize=None)(build_case)  # the table's cases: built once, shared, never modified


def table_case(shape):
    return case(*shape, TABLE[shape][1])


def addend(c):
    return ADD_STEP * c["r"].to(F64)        # units of 2^-s


def pre_act(c):
    return GB_STEP * c["pre"].to(F64)       # values


def saved_grad(c):
    return c["saved"].to(F64)


def linear_refs(c, ring):
    """EPI 0, 1, 4, 5, 6 in units of 2^-s (integers): float64 values that are bf16-exact."""
    p, bias, r = c["p"], c["bias"], addend(c)
    kr = keep_bits(c["mask"], c["M"], c["N"]) * r
    if ring:  # the addend joins the bf16-staged tile: two roundings
        return {0: rne(p), 1: rne(p + bias), 4: rne(rne(p) + r), 5: rne(rne(p + bias) + r), 6: rne(rne(p) + kr)}
    return {0: rne(p), 1: rne(p + bias), 4: rne(p + r), 5: rne(p + bias + r), 6: rne(p + kr)}


def gelu_arg(c, ring):
    """The GELU argument's GEMM part as the mainloop's epilogue sees it: f(RNE(P)) or the fp32 P."""
    pv = c["p"] * c["u"]
    return rne(pv) if ring else pv


def saved_refs(c):
    """EPI 8: d = P Y exactly, dx = RNE(d), db = RNE(sum d), db_out: RNE(base + sum d); the per-column
    exactness bound sum_m |d| * 4 (units of 2^-s) < 2^24."""
    d = c["p"] * saved_grad(c)                                      # units of 2^-s, multiples of 1/4
    assert bool((4 * d == (4 * d).round()).all())
    worst = float((4 * d).abs().sum(0).max()) + 4 * DB_BASE_MAX
    assert worst < LIM, f"EPI 8 column sums are not exact in fp32: {worst:.0f} >= 2^24"
    col = d.sum(0)
    return dict(dx=rne(d), db=rne(col), db_acc=rne(c["base"] + col), worst=worst)


@functools.lru_cache(maxsize=None)
def stats_case(M, N, K):
    """EPI 9: integer operands, A column 0 constant."""
    seed = (M * 5 + N * 11 + K) % (1 << 31)
    a, b = ints((M, K), STATS_A_MAX, seed), ints((N, K), A_MAX, seed + 1)
    a[:, 0] = STATS_A0
    assert (K - 1) * STATS_A_MAX * A_MAX + STATS_A0 * A_MAX < LIM
    c = rne(a @ b.t() + 0.0)
    # the shifted sums (x - x0) and their merges over a group of <= 256 rows: integers below 2^24
    assert 2 * 256 * float(c.abs().max()) < LIM
    return dict(a=a, b=b, c=c)


# ---------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------
def dev(t, scale=1.0):
    """A float64 CPU tensor (times an exact power of two) as a fresh bf16 device tensor."""
    return as_bf16(t * scale).cuda()


def record(line):
    """One line for the results file (profiles/r10_gemm_nt_exact_tests.md is written from these)."""
    print(f"[exact] {line}")


def poison(*shapes):
    """NaN-filled blocks of the outputs' sizes, freed again: an element a kernel leaves unwritten is
    then unlikely to read as a previous correct result."""
    junk = [torch.full(s, float("nan"), dtype=BF16, device="cuda") for s in shapes]
    del junk


class impl_of:
    """gemm_nt_impl(impl) for the block, the previous selection restored after it."""

    def __init__(self, m, shape):
        self.m, self.impl = m, TABLE[shape][0] if shape in TABLE else 1

    def __enter__(self):
        self.prev = self.m.gemm_nt_impl(self.impl)

    def __exit__(self, *exc):
        self.m.gemm_nt_impl(self.prev)


def check_path(m, shape):
    """The mainloop the table lists the shape for is the one the host code selects."""
    M, N, K = shape
    ring = on_ring(shape)
    assert m.gemm_nt_supported(M, N, K)
    assert m.gemm_nt_stats_rows(K) == (256 if ring else 128), (shape, "mainloop selection")
    assert bool(m.gemm_nt_epi_ok(M, N, K)) == (not ring)
    return ring


# ---------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------
def run_linear(m, c, ring, what, epis=(0, 1, 4, 5, 6)):
    M, N, u = c["M"], c["N"], c["u"]
    a, b = dev(c["a"]), dev(c["b"], u)
    bias, r, mask = dev(c["bias"], u), dev(addend(c), u), c["mask"].cuda()
    want = linear_refs(c, ring)
    for epi in epis:
        if epi <= 1:
            out = torch.full((M, N), float("nan"), dtype=BF16, device="cuda")
            got = m.gemm_nt(a, b, bias if epi else None, out=out)
            assert got.data_ptr() == out.data_ptr()
        else:
            poison((M, N))
            got = m.gemm_nt_add(a, b, r, bias if epi == 5 else None, mask if epi == 6 else None)
        check_bits(got, as_bf16(want[epi] * u), f"{what} EPI {epi}")


@pytest.mark.parametrize("shape", list(TABLE), ids=sid)
def test_linear_epilogues_exact(shape):
    """EPI 0, 1 (into a NaN-filled out=), 4, 5, 6: every bit of RNE(...) as the mainloop's contract
    nests it — two roundings on the ring, one on the 4-wave loop."""
    m, c = _m(), table_case(shape)
    with impl_of(m, shape):
        ring = check_path(m, shape)
        record(f"linear {sid(shape)}: {'ring' if ring else '4-wave'} — {TABLE[shape][2]}")
        run_linear(m, c, ring, f"gemm_nt {sid(shape)}")


@pytest.mark.parametrize("shape", list(TABLE), ids=sid)
def test_gelu_epilogues(shape):
    """EPI 2: C = RNE(P) to the bit, Y within the neighbour / band rule of gelu(argument + bias) with
    the mainloop's own argument.  EPI 7 (4-wave only; the ring declines and raises): C ~ gelu'(x),
    Y ~ gelu(x), x = P + bias."""
    m, c = _m(), table_case(shape)
    M, N, u = c["M"], c["N"], c["u"]
    a, b, gbias = dev(c["a"]), dev(c["b"], u), dev(c["gbias"])
    what = f"gemm_nt_gelu {sid(shape)}"
    with impl_of(m, shape):
        ring = check_path(m, shape)
        x = gelu_arg(c, ring) + c["gbias"]
        assert float(x.abs().max()) <= X_LIMIT
        poison((M, N), (M, N))
        pre, y = m.gemm_nt_gelu(a, b, gbias)
        check_bits(pre, as_bf16(rne(c["p"]) * u), f"{what} EPI 2 C")
        check_activation(y, gelu64(x), f"{what} EPI 2 Y")
        if ring:
            with pytest.raises(RuntimeError, match="-4"):
                m.gemm_nt_gelu(a, b, gbias, saved_grad=True)
            return
        x = c["p"] * u + c["gbias"]
        poison((M, N), (M, N))
        gd, y = m.gemm_nt_gelu(a, b, gbias, saved_grad=True)
        check_activation(gd, gelu_grad64(x), f"{what} EPI 7 C")
        check_activation(y, gelu64(x), f"{what} EPI 7 Y")


@pytest.mark.parametrize("shape", list(TABLE), ids=sid)
def test_dgelu_epilogue_and_bias_gradient(shape):
    """EPI 3: dx within the neighbour / band rule of argument * gelu'(pre + bias); db against the
    float64 column sum of the unrounded reference, per column within
    ulp_bf16(ref) / 2 + (DELTA + M 2^-24) sum |d_ref|."""
    m, c = _m(), table_case(shape)
    M, N, u = c["M"], c["N"], c["u"]
    a, b, gbias, pre = dev(c["a"]), dev(c["b"], u), dev(c["gbias"]), dev(pre_act(c))
    what = f"gemm_nt_dgelu {sid(shape)}"
    with impl_of(m, shape):
        ring = check_path(m, shape)
        x = pre_act(c) + c["gbias"]
        assert float(x.abs().max()) <= X_LIMIT
        d = gelu_arg(c, ring) * gelu_grad64(x)
        poison((M, N), (N,))
        dx, db = m.gemm_nt_dgelu(a, b, pre, gbias)
    check_activation(dx, d, f"{what} EPI 3 dx")
    ref, bound = d.sum(0), db_bound(d.sum(0), d.abs().sum(0), M)
    db = db.cpu()
    assert db.dtype == BF16 and db.shape == (N,)
    ratio = (db.to(F64) - ref).abs() / bound
    worst = float(ratio.max())
    record(f"{what} EPI 3 db: worst |err| / bound = {worst:.3e}")
    assert bool(torch.isfinite(db.float()).all()) and worst <= 1.0, \
        f"{what} db: column {int(ratio.argmax())} (tile column {int(ratio.argmax()) // 256}): got " \
        f"{float(db[ratio.argmax()])!r}, float64 {float(ref[ratio.argmax()])!r}, |err| / bound {worst:.3f}"


def run_saved(m, c, what):
    M, N, u = c["M"], c["N"], c["u"]
    want = saved_refs(c)
    a, b, y, bias = dev(c["a"]), dev(c["b"], u), dev(saved_grad(c)), dev(c["gbias"])
    poison((M, N), (N,))
    dx, db = m.gemm_nt_dgelu(a, b, y, bias, saved_grad=True)
    check_bits(dx, as_bf16(want["dx"] * u), f"{what} EPI 8 dx")
    check_bits(db.view(1, N), as_bf16(want["db"] * u).view(1, N), f"{what} EPI 8 db")
    acc = dev(c["base"], u)
    poison((M, N))
    (dx2,) = m.gemm_nt_dgelu(a, b, y, bias, db_out=acc, saved_grad=True)
    check_bits(dx2, as_bf16(want["dx"] * u), f"{what} EPI 8 dx (db_out=)")
    check_bits(acc.view(1, N), as_bf16(want["db_acc"] * u).view(1, N), f"{what} EPI 8 db_out")
    return want["worst"]


@pytest.mark.parametrize("shape", list(TABLE), ids=sid)
def test_saved_gelu_grad_epilogue_exact(shape):
    """EPI 8 (4-wave only): dx = RNE(P Y) and db = RNE(sum) / RNE(base + sum) to the bit — a partial
    row lost, doubled or written to another slot changes db.  The ring declines (-4) and raises."""
    m, c = _m(), table_case(shape)
    with impl_of(m, shape):
        if check_path(m, shape):
            a, b = dev(c["a"]), dev(c["b"], c["u"])
            with pytest.raises(RuntimeError, match="-4"):
                m.gemm_nt_dgelu(a, b, dev(saved_grad(c)), dev(c["gbias"]), saved_grad=True)
            return
        worst = run_saved(m, c, f"gemm_nt_dgelu {sid(shape)}")
        record(f"saved-grad {sid(shape)}: largest sum |d| * 4 * 2^s = {worst:.0f} ({worst / LIM:.3f} of 2^24)")


@pytest.mark.parametrize("shape", [s for s in TABLE if not (on_ring(s) and s[1] % 256)], ids=sid)
def test_stats_epilogue(shape):
    """EPI 9: C = RNE(P) to the bit, each group's sum exactly the sum of the bf16 outputs, its centred
    sum of squares within the project's tolerance for per-group partials."""
    m = _m()
    M, N, K = shape
    c = stats_case(M, N, K)
    with impl_of(m, shape):
        ring = check_path(m, shape)
        rows = m.gemm_nt_stats_rows(K)
        poison((M, N))
        out, part = m.gemm_nt_stats(dev(c["a"]), dev(c["b"]))
    what = f"gemm_nt_stats {sid(shape)}"
    check_bits(out, as_bf16(c["c"]), f"{what} C")
    assert part.shape == (M // rows, 2, N) and rows == (256 if ring else 128)
    record(f"{what}: {rows}-row groups x {M // rows}")
    check_tile_stats(part, out.view(M, 1, 1, N).permute(0, 3, 1, 2), N, rows, what)


def test_persistent_grid_two_tiles_per_workgroup():
    """More tiles than workgroups, not a multiple of them, with a half-width tile column: some
    workgroups run two tiles and halfn changes between them.  EPI 0, 5 and 8."""
    m = _m()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    N, K = PERSISTENT_NK
    M = persistent_rows(cus)
    tiles_m, tiles_n = M // 256, -(-N // 256)
    tiles, grid = tiles_m * tiles_n, cus // 8 * 8
    assert tiles > cus and tiles % cus != 0 and N % 256 == 128
    change = [v for v in range(tiles - grid)
              if (nt4_tile_coords(v, tiles_m, tiles_n)[1] == tiles_n - 1)
              != (nt4_tile_coords(v + grid, tiles_m, tiles_n)[1] == tiles_n - 1)]
    assert change, "no workgroup changes halfn between its tiles"
    record(f"persistent {M}x{N}x{K}: {tiles} tiles on {grid} workgroups, {len(change)} change halfn")
    c = build_case(M, N, K, PERSISTENT_S, PERSISTENT_B_MAG)  # large: not cached
    prev = m.gemm_nt_impl(1)
    try:
        assert m.gemm_nt_stats_rows(K) == 128
        run_linear(m, c, False, f"gemm_nt {M}x{N}x{K}", epis=(0, 5))
        run_saved(m, c, f"gemm_nt_dgelu {M}x{N}x{K}")
    finally:
        m.gemm_nt_impl(prev)


def sentinel(M, N):
    return (torch.arange(M * N, dtype=torch.float32, device="cuda").reshape(M, N) % 251 - 125.5).to(BF16)


@pytest.mark.parametrize("M,N,K,impl,why", [(320, 256, 64, 1, "M % 256 != 0"), (256, 256, 96, 1, "K % 64 != 0"),
                                            (256, 384, 256, 0, "N % 256 = 128 on the ring")])
def test_unsupported_shapes_raise_and_keep_out(M, N, K, impl, why):
    m = _m()
    prev = m.gemm_nt_impl(impl)
    try:
        assert not m.gemm_nt_supported(M, N, K), why
        a, b = torch.ones(M, K, dtype=BF16, device="cuda"), torch.ones(N, K, dtype=BF16, device="cuda")
        out, bias = sentinel(M, N), torch.ones(N, dtype=BF16, device="cuda")
        for bs in (None, bias):
            with pytest.raises(RuntimeError):
                m.gemm_nt(a, b, bs, out=out)
        with pytest.raises(RuntimeError):
            m.gemm_nt_add(a, b, out)
        torch.cuda.synchronize()
        assert same_bits(out, sentinel(M, N)), why
    finally:
        m.gemm_nt_impl(prev)


def test_epilogue_rejections_raise():
    """The saved-gelu' pair and half-width statistics at K = 128 (the ring), a mask of the wrong
    length and a mask together with a bias: each binding raises; the addend keeps its bits."""
    m = _m()
    K = 128
    a, b = torch.ones(256, K, dtype=BF16, device="cuda"), torch.ones(256, K, dtype=BF16, device="cuda")
    bias, r = torch.ones(256, dtype=BF16, device="cuda"), sentinel(256, 256)
    with pytest.raises(RuntimeError, match="-4"):
        m.gemm_nt_gelu(a, b, bias, saved_grad=True)
    with pytest.raises(RuntimeError, match="-4"):
        m.gemm_nt_dgelu(a, b, r, bias, saved_grad=True)
    acc = bias.clone()
    with pytest.raises(RuntimeError, match="-4"):
        m.gemm_nt_dgelu(a, b, r, bias, db_out=acc, saved_grad=True)
    with pytest.raises(RuntimeError):
        m.gemm_nt_stats(a, torch.ones(384, K, dtype=BF16, device="cuda"))
    good = torch.full((256 * 256 // 8,), 255, dtype=torch.uint8, device="cuda")
    for mask in (good[:-1], torch.cat([good, good[:1]])):
        with pytest.raises(RuntimeError, match="mask"):
            m.gemm_nt_add(a, b, r, None, mask)
    with pytest.raises(RuntimeError, match="exclusive"):
        m.gemm_nt_add(a, b, r, bias, good)
    torch.cuda.synchronize()
    assert same_bits(r, sentinel(256, 256)) and same_bits(acc, bias)
