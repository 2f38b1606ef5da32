"""Per-element float64 and bit-exact checks of layernorm.hip, gelu.hip and embed.hip, called straight
through the extension.  The builders, references and checkers below run on the CPU and are validated
(and shown to reject perturbed references) by test_ln_gelu_embed_cpu.py.

U = 2^-24 is the fp32 unit roundoff; n = 8 VPL is the number of terms a lane sums sequentially
(VPL = vectors of 8 per lane, ceil(C / 512), 7 -> 8).  All bounds are first order in U and carry a
factor 1 + 2^-10 for the higher-order terms.

LayerNorm forward (ln_fwd_kernel), counted from its operation sequence.  v is the fp32 row: the
bf16 x, or the fp32 sum (x + r) (+ rbias) in that order — sums of bf16 values, reproduced
exactly in torch; the stored h must be RNE(v) bit for bit, and the float64 reference of mean, rstd
and y is the LayerNorm OF THAT fp32 v (not of the stored bf16 h), so the band below needs no term for
the residual sum.  A = mean_j |v_j|.

    mean   n - 1 lane additions (the first adds to 0), 6 shuffle additions, 1/C (one rounding, a
           second allowed for a division that is not correctly rounded), one multiply:
               |mean - mu| <= K_MEAN U A,                 K_MEAN = 8 VPL + 8
    rstd   per term d = v - mean (1), d d (1), the addition (n lane + 6 shuffle in all): the sum of
           squares is (n + 8) U relative (its terms are positive); 1/C and the multiply (2), + eps
           and the rounding of eps itself (2) make var + eps (n + 12) U relative, halved by the
           inverse square root, plus 2 U for the 1-ulp hardware rsqrt:
               |rstd - ref| / ref <= (K_RSTD + X) U,      K_RSTD = 4 VPL + 8
           X is the second-order effect of the mean's own error on the centred sum,
           (K_MEAN U A)^2 / (2 (var + eps) U) per row: below 1 for normal rows, it matters for
           |mean| >> std; test_ln_gelu_embed_cpu.py asserts K_RSTD + X + 4 <= K_Y for every row.
    y      o = (v - mean) rstd w + b: subtraction, two multiplies, one addition (or an fma) on
           top of the errors of mean and rstd:
               |o - y64| <= U (|w| rstd (|v - mu| (4 + K_RSTD + X) + K_MEAN A) + |b|)
                         <= K_Y U ((|v - mu| + A) rstd |w| + |b|),   K_Y = 8 VPL + 16
           The count needs max(4 VPL + 12 + X, 8 VPL + 8), so K_Y holds with 8 to spare.  y follows
           the neighbour / band rule of check_activation with this ABSOLUTE band (check_banded).

The band rule with an absolute band.  The kernel stores RNE(o) of an fp32 o within `band` of the
float64 v, and RNE is monotonic, so the stored value lies between RNE(v - band) and RNE(v + band).
Where the band reaches no rounding midpoint the two are equal and the output must be RNE(v) bit for
bit; where it reaches one, either neighbour passes: check_activation's rule.  An absolute band can
exceed the bf16 spacing of a small output (y near zero in a row with |mean| >> std, a dx left by
cancellation); the interval form is the same rule without the assumption band < spacing / 2.  It
must not go vacuous: the band spans more than two bf16 values only where |v| is below about 2^8
band, a small fraction of the elements whose band reaches a midpoint at all, so that share is capped
at WIDE_CAP of the random rows and of every dx (asserted on the CPU and in the GPU tests).

LayerNorm backward (ln_bwd_kernel), against the float64 formula built from the kernel's OWN stored
mean / rstd (mu, rs), so forward error is not charged twice.  g = dy w is exact in fp32 (8 x 8 bits).
xh = (x - mu) rs carries 2 U.  s1 = mean(g): (n + 7) U mean|g|; s2 = mean(g xh): (n + 10) U
mean|g xh|.  o = (g - s1 - xh s2) rs (+ dres): the subtraction g - s1 (1), the product xh s2 (1 +
the 2 of xh), the second subtraction (1), the multiply by rs (1), the final addition (1):
    |o - o64| <= K_B U (rs (|g| + G1 + |xh| G2) + |dres|),  K_B = 8 VPL + 16,
    G1 = mean_j |g_j|, G2 = mean_j |g_j xh_j|   (the largest coefficient, on |xh| G2, is n + 16)
dbeta sums dy itself: with integer dy in [-8, 8] every partial sum is exact and dbeta = RNE(sum dy)
bit for bit, whatever the order.  With random dy, and for dgamma (terms dy xh, 3 U each) and drbias
(terms the UNROUNDED fp32 o, each within its dx band; not the stored bf16 dx), the output must lie
between the bf16 roundings of sum -+ bound, bound = sum of the per-term errors + rows U sum|term|
(at most rows - 1 additions of non-zero values touch a column: wave registers, the in-block LDS
combine, then colsum's tree).  The arena form accumulates in fp32 onto the bf16 base before the one
rounding (one more U (|base| + sum|term|)).

bias + GELU.  The argument is the fp32 sum x + b, reproduced exactly.  The reference is the tanh
GELU in its logistic form x sigma(2u), mathematically the same function as gelu64 but without its
cancellation: 1 + tanh(u) moves in steps of 2^-53, percent-wrong at x = -7 and exactly 0 from x = -7.5
on, for values the kernel resolves (test_ln_gelu_embed_cpu.py compares the two).  For |x + b| <= 8
the rule is check_activation's with the project's DELTA = 2^-14.  db: db_bound per column.  The bias
is a multiple of 2^-6 in [-1.5, 1.5] that repeats with a period of 193 columns (bf16 holds no 4096
distinct such values): it differs between any two columns whose distance is no multiple of 193, which
covers every shift by a whole number of vectors below 193 vectors, a wrong period F8 among them.

Contract of gelu_sig / gelu_sig_grad over all bf16 inputs (test_gelu_every_bf16_pattern):
    |x + b| <= 8          the band rule; only bf16-subnormal results (|v| < 2^-126, from inputs
                          below 2^-125) are held to the next rule instead: they may be flushed
    8 < |x + b| <= 2^40   finite, |got - v| <= 2^-8 |v| + 2^-120; the floor covers x near -10,
                          where the reciprocal 1 / (1 + e) is subnormal and may be flushed
    beyond 2^40           outside the contract, not asserted: an fp32 emulation of gelu_sig_grad on
                          the CPU first goes non-finite at x = -1.17e13 (x w overflows) and
                          x = 1.8e19 (x^2 overflows); the forward stays finite everywhere.  That is
                          an emulation, not a hardware measurement.

Embedding.  All four kernels add in a fixed order without multiplies, so the host reproduces them to
the bit: embed_fwd RNE(wte[id] + wpe[s]); embed_bwd with integer dy (any atomic order is exact);
dwpe the fp32 sum over b in order; embed_bwd_sorted by sorted_reference, which follows the documented
piece order; order_pins makes that order visible after the bf16 rounding.
Ids >= Vp sort last, so they and a run of a valid id that reaches row N - 1 cannot share one id
pattern: hence two patterns at N = 785.

Measured on an MI355X (each test prints its figures; 89 tests, 5 s, the slowest 0.5 s).  Worst error
as a share of the counted bound: mean 0.061 (an offset row; 0.008 on normal rows), rstd 0.183 (the
last-bit row at C = 4096; 0.13 on normal rows); dgamma 0.014 and drbias 0.006 beyond the output's own
rounding; db of bias_gelu_bwd 0.12 - 0.97 (db_bound includes that rounding).  y and dx are not the
nearest bf16 value in 165 of 3.9 M elements, each inside its band.  Band shares (CPU): at most 1.27 %
on random rows (one of 8 elements at (1, 8)), 1.6 - 6.7 % on the offset rows, 17 - 39 % on the last-bit
rows; bands spanning more than two values: at most 0.12 % on random rows, 0.95 % on offset rows.  Every
finite bf16 input: gelu_sig is finite everywhere, the relative rule's worst case is 0.996 of its bound
(the output's own rounding); gelu_sig_grad worst 0.876, and non-finite only beyond 2^40 (19030
patterns).
"""
import functools

import numpy as np
import pytest
import torch

from test_gemm_dw_exact_gpu import check_bits, same_bits
from test_gemm_nt_exact_gpu import (GB_STEP, _quantum, activation_expect, as_bf16, check_activation, classify,
                                    db_bound, rne)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -24
HO = 1.0 + 2.0 ** -10   # higher-order terms of the first-order bounds
EPS = 1e-5


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def record(line):
    print(f"[ln-gelu-embed] {line}")


def q16(t):
    """Any float tensor rounded to bf16 values, as float64."""
    return t.to(torch.float32).to(BF16).to(F64)


def randn16(shape, gen, scale=1.0):
    return q16(torch.randn(shape, generator=gen, dtype=torch.float32) * scale)


def dev(t):
    return as_bf16(t).cuda()


def interval_ok(got, s, bound):
    """got (bf16 values as float64) lies between the bf16 roundings of s - bound and s + bound."""
    return (got >= rne(s - bound)) & (got <= rne(s + bound))


def share_ok(count, n, cap):
    """count of n elements is within the share cap; below SMALL_CASE elements, where one element is
    more than the cap, one is allowed."""
    return count <= cap * n or (n < SMALL_CASE and count <= 1)


def wide_count(v, band, rows=None):
    """Number of elements whose band spans more than two bf16 values."""
    if rows is not None:
        v, band = v[rows], band[rows]
    return int(((rne(v + band) - rne(v - band)) > 1.5 * _quantum(v)).sum())


def check_banded(got, v, band, what, wide_cap=None):
    """The neighbour / band rule for an absolute band (module docstring): every element of the bf16
    `got` lies between RNE(v - band) and RNE(v + band) — so it is RNE(v) itself wherever the band
    reaches no rounding midpoint.  wide_cap: largest share of elements whose band may span more than
    two values."""
    got = got.cpu()
    assert got.dtype == BF16 and got.shape == v.shape, (what, got.dtype, got.shape)
    g, near = got.double(), rne(v)
    lo, hi = rne(v - band), rne(v + band)
    ok = (g >= lo) & (g <= hi)
    wide = wide_count(v, band)
    record(f"{what}: not the nearest in {int((ok & (g != near)).sum())} of {v.numel()} (the band reaches a "
           f"midpoint in {float((lo != hi).double().mean()):.3%}, spans more than two values in {wide} elements)")
    assert wide_cap is None or share_ok(wide, v.numel(), wide_cap), \
        f"{what}: {wide} of {v.numel()} bands span more than two values"
    check_bits(got, torch.where(ok, got, as_bf16(near)), what)


# ---------------------------------------------------------------------------------------------
# LayerNorm: cases and float64 references (CPU)
# ---------------------------------------------------------------------------------------------
LN_FWD = [
    (1, 8, "one lane, three idle waves"),
    (7, 512, "VPL 1 full"),
    (5, 520, "VPL 2, one lane in the second vector"),
    (37, 776, "general ragged case"),
    (6, 1600, "VPL 4 ragged"),
    (5, 2048, "VPL 4 full"),
    (3, 2056, "VPL 5"),
    (3, 3072, "VPL 6"),
    (3, 3080, "VPL 7 -> 8, one empty vector"),
    (2, 4096, "VPL 8 full"),
]
LN_ADV_C = (512, 776, 2048, 3080, 4096)   # adversarial rows among random rows; 512, 2048, 4096: constant row exact
LN_FORMS = ("plain", "add", "add_rbias")
LN_BWD = [s[:2] for s in LN_FWD if s[1] <= 2048] + [(8197, 64), (1, 64), (5, 64)]
# (8197, 64): the grid is capped at 512 blocks = 2048 waves, 4 rows per wave and a fifth for the first
# five waves, so the prefetch condition row + nw < N is false and true inside one launch;
# (1, 64), (5, 64): one / two blocks whose other waves have no row and still join the LDS combine
OFFSET = 16.0      # |mean| / std of the offset rows; band share of those rows <= OFFSET_CAP (CPU test)
RANDOM_CAP, OFFSET_CAP = 0.02, 0.10   # largest share of elements whose band reaches a rounding midpoint
WIDE_CAP = RANDOM_CAP / 4             # ... whose band spans more than two values (random rows, every dx)
SMALL_CASE = 50                       # below 1 / RANDOM_CAP elements one element in the band is allowed
ADV_ROWS = {1: "offset", 2: "needle", 3: "constant", 4: "lastbit", 6: "offset"}  # rows 0, 5, 7: random
ADV_N = 8
CONST_VALUE = 1.5


def vpl_for(C):
    v = (C + 511) // 512
    return 8 if v == 7 else v


def k_mean(C):
    return 8 * vpl_for(C) + 8


def k_rstd(C):
    return 4 * vpl_for(C) + 8


def k_y(C):
    return 8 * vpl_for(C) + 16


def k_bwd(C):
    return 8 * vpl_for(C) + 16


def adversarial_rows(C, gen):
    """[ADV_N, C] bf16 values: random-normal rows with the ADV_ROWS among them."""
    x = randn16((ADV_N, C), gen)
    x[1] = q16(OFFSET + torch.randn(C, generator=gen))          # |mean| >> std: a one-pass variance fails rstd
    x[6] = q16(-OFFSET + torch.randn(C, generator=gen))
    x[2] = 0.0
    x[2, (5 * C // 7) | 1] = 3.0                                # one needle in a zero row
    x[3] = CONST_VALUE                                          # constant: mean exact, y = b at power-of-two C
    x[4] = 1.0 + 2.0 ** -7 * torch.randint(0, 2, (C,), generator=gen).to(F64)  # differ in the last bf16 bit only
    return x


@functools.lru_cache(maxsize=None)
def ln_case(N, C, form, adv=False):
    """Inputs (float64 tensors of bf16 values), the fp32 row v the kernel normalises, and the float64
    references.  Shared by the tests; never modified."""
    gen = torch.Generator().manual_seed(1000003 * N + 17 * C + LN_FORMS.index(form) + (7919 if adv else 0))
    x = adversarial_rows(C, gen) if adv else randn16((N, C), gen)
    N = x.shape[0]
    c = dict(N=N, C=C, form=form, adv=adv, x=x, w=randn16((C,), gen), b=randn16((C,), gen), r=None, rb=None)
    v32 = x.to(torch.float32)
    if form != "plain":
        r = randn16((N, C), gen)
        if adv:
            r[list(ADV_ROWS)] = 0.0     # the adversarial rows reach the statistics unchanged
        c["r"] = r
        v32 = v32 + r.to(torch.float32)
        if form == "add_rbias":
            c["rb"] = randn16((C,), gen)
            v32 = v32 + c["rb"].to(torch.float32)
    c["v32"] = v32
    c.update(ln_reference(v32.to(F64), c["w"], c["b"]))
    return c


def ln_reference(v, w, b, one_pass_row=None):
    """The textbook two-pass LayerNorm in float64 with the error bounds of the module docstring.
    one_pass_row: that row's variance as fl32(E[v^2]) - fl32(mean)^2 in fp32 (the CPU file uses it
    to show that the checks reject a one-pass kernel)."""
    N, C = v.shape
    mu = v.mean(1, keepdim=True)
    var = ((v - mu) ** 2).mean(1, keepdim=True)
    if one_pass_row is not None:
        f = v[one_pass_row].to(torch.float32)
        m32 = f.sum() / C
        var[one_pass_row] = float((f * f).sum() / C - m32 * m32)
    rstd = 1.0 / torch.sqrt(var + EPS)
    A = v.abs().mean(1, keepdim=True)
    y = (v - mu) * rstd * w + b
    extra = (k_mean(C) * U * A) ** 2 / (2.0 * (var + EPS) * U)
    return dict(mu=mu[:, 0], rstd=rstd[:, 0], y=y, A=A[:, 0], extra=extra[:, 0],
                mean_bound=k_mean(C) * U * A[:, 0] * HO,
                rstd_bound=(k_rstd(C) + extra[:, 0]) * U * HO,
                band=k_y(C) * U * ((v - mu).abs() + A) * rstd * w.abs() + k_y(C) * U * b.abs())


def band_share(v, band, rows=None):
    """Share of the elements whose float64 value lies inside the ambiguity band."""
    if rows is not None:
        v, band = v[rows], band[rows]
    return float(classify(v, band=band)[3].double().mean())


def check_ln_forward(c, mean, rstd, y, h, what):
    """mean, rstd (fp32), y, h (bf16) of the kernel, on the CPU, against the case's references."""
    N, C = c["N"], c["C"]
    mean, rstd = mean.double(), rstd.double()
    e_mean = (mean - c["mu"]).abs()
    r_mean = float((e_mean / c["mean_bound"].clamp_min(1e-300)).max())
    r_rstd = float(((rstd - c["rstd"]).abs() / c["rstd"] / c["rstd_bound"]).max())
    record(f"{what}: worst / bound: mean {r_mean:.3f}, rstd {r_rstd:.3f} (K_MEAN {k_mean(C)}, K_RSTD {k_rstd(C)}, "
           f"largest X {float(c['extra'].max()):.2f}, K_Y {k_y(C)})")
    assert bool((e_mean <= c["mean_bound"]).all()), f"{what}: mean off by {r_mean:.3f} of its bound"
    assert r_rstd <= 1.0, f"{what}: rstd off by {r_rstd:.3f} of its bound"
    if h is not None:
        check_bits(h, c["v32"].to(BF16), f"{what} h")
    check_banded(y, c["y"], c["band"], f"{what} y", wide_cap=None if c["adv"] else WIDE_CAP)
    if c["adv"] and C & (C - 1) == 0:
        k = [r for r, kind in ADV_ROWS.items() if kind == "constant"][0]
        assert float(mean[k]) == CONST_VALUE, f"{what}: the constant row's mean is {float(mean[k])!r}"
        assert same_bits(y[k].cpu(), as_bf16(c["b"])), f"{what}: y of the constant row is not b"


@functools.lru_cache(maxsize=None)
def ln_bwd_inputs(N, C, integer_dy):
    gen = torch.Generator().manual_seed(2000003 * N + 31 * C + int(integer_dy))
    dy = torch.randint(-8, 9, (N, C), generator=gen).to(F64) if integer_dy else randn16((N, C), gen)
    return dict(x=randn16((N, C), gen), dy=dy, w=randn16((C,), gen), b=randn16((C,), gen),
                dres=randn16((N, C), gen), base=randn16((3, C), gen, 4.0))


def ln_bwd_reference(x, dy, w, mu, rs, dres):
    """float64 LayerNorm backward from given per-row mean / rstd (float64 [N]); dres may be None."""
    N, C = x.shape
    mu, rs = mu[:, None], rs[:, None]
    xh = (x - mu) * rs
    g = dy * w
    G1, G2 = g.abs().mean(1, keepdim=True), (g * xh).abs().mean(1, keepdim=True)
    o = (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)) * rs
    band = rs * (g.abs() + G1 + xh.abs() * G2)
    if dres is not None:
        o, band = o + dres, band + dres.abs()
    band = k_bwd(C) * U * band * HO
    tw = dy * xh
    return dict(dx=o, band=band,
                dgamma=(tw.sum(0), (3 * U + N * U) * tw.abs().sum(0) * HO),
                dbeta=(dy.sum(0), N * U * dy.abs().sum(0) * HO),
                drbias=(o.sum(0), (band.sum(0) + N * U * o.abs().sum(0)) * HO),
                abs=dict(dgamma=tw.abs().sum(0), dbeta=dy.abs().sum(0), drbias=o.abs().sum(0)))


# ---------------------------------------------------------------------------------------------
# LayerNorm: GPU tests
# ---------------------------------------------------------------------------------------------
def run_ln_forward(m, c):
    x, w, b = dev(c["x"]), dev(c["w"]), dev(c["b"])
    if c["form"] == "plain":
        y, mean, rstd = m.layernorm_fwd(x, w, b, EPS)
        h = None
    else:
        rb = dev(c["rb"]) if c["rb"] is not None else None
        h, y, mean, rstd = m.add_layernorm_fwd(x, dev(c["r"]), w, b, EPS, rb)
        h = h.cpu()
    return mean.cpu(), rstd.cpu(), y.cpu(), h


@pytest.mark.parametrize("form", LN_FORMS)
@pytest.mark.parametrize("N,C,why", LN_FWD, ids=[f"{s[0]}x{s[1]}" for s in LN_FWD])
def test_layernorm_forward(cuda, N, C, why, form):
    """mean / rstd per row within the counted bounds, h = RNE(fp32 sum) bit for bit, y per element by
    the neighbour / band rule against the float64 LayerNorm of the fp32 h (module docstring)."""
    c = ln_case(N, C, form)
    check_ln_forward(c, *run_ln_forward(_m(), c), f"ln_fwd {form} {N}x{C} ({why})")


@pytest.mark.parametrize("form", ("plain", "add"))
@pytest.mark.parametrize("C", LN_ADV_C)
def test_layernorm_forward_adversarial_rows(cuda, C, form):
    """Offset rows (|mean| = 16 std), a needle row, a constant row and a last-bit row among random
    rows: same checks; at power-of-two C the constant row's mean is exact and its y equals b."""
    c = ln_case(ADV_N, C, form, adv=True)
    check_ln_forward(c, *run_ln_forward(_m(), c), f"ln_fwd {form} adversarial C={C}")


def check_colgrad(name, got, ref, what, base=None):
    s, bound = ref[name]
    if base is not None:
        bound = bound + U * (base.abs() + ref["abs"][name])
        s = s + base
    got = got.cpu().double()
    bad = ~interval_ok(got, s, bound)
    assert not bool(bad.any()), f"{what} {name}: column {int(bad.nonzero()[0])} outside the interval"
    # what the output's own rounding (half a bf16 spacing) does not explain, as a share of the bound
    return float((((got - s).abs() - 0.5 * _quantum(s)).clamp_min(0.0) / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("form", LN_FORMS)
@pytest.mark.parametrize("N,C", LN_BWD, ids=[f"{n}x{c}" for n, c in LN_BWD])
def test_layernorm_backward(cuda, N, C, form):
    """dx per element (band rule, from the kernel's own mean / rstd), dgamma / dbeta / drbias per
    column (interval rule), dbeta = RNE(sum dy) bit for bit for integer dy, and the arena form
    grads=[...] accumulated onto a non-zero base."""
    m = _m()
    for integer_dy in (False, True):
        i = ln_bwd_inputs(N, C, integer_dy)
        x, dy, w, b = dev(i["x"]), dev(i["dy"]), dev(i["w"]), dev(i["b"])
        dres = None if form == "plain" else i["dres"]
        _, mean, rstd = m.layernorm_fwd(x, w, b, EPS)
        ref = ln_bwd_reference(i["x"], i["dy"], i["w"], mean.cpu().double(), rstd.cpu().double(), dres)
        names = ["dgamma", "dbeta"] + (["drbias"] if form == "add_rbias" else [])

        def call(grads=None):
            if form == "plain":
                return m.layernorm_bwd(dy, x, w, mean, rstd, grads)
            return m.layernorm_bwd_add(dy, x, w, mean, rstd, dev(dres), form == "add_rbias", grads)

        outs = call()
        what = f"ln_bwd {form} {N}x{C} {'integer' if integer_dy else 'normal'} dy"
        assert len(outs) == 1 + len(names)
        check_banded(outs[0], ref["dx"], ref["band"], f"{what} dx", wide_cap=WIDE_CAP)
        worst = {name: check_colgrad(name, outs[1 + k], ref, what) for k, name in enumerate(names)}
        if integer_dy:
            check_bits(outs[2].cpu().reshape(1, C), as_bf16(rne(ref["dbeta"][0])).reshape(1, C), f"{what} dbeta exact")
        base = i["base"][:len(names)]
        dests = [dev(row) for row in base]
        o2 = call(dests)
        assert len(o2) == 1 and same_bits(o2[0], outs[0])
        onto = {name: check_colgrad(name, dests[k], ref, what, base=base[k]) for k, name in enumerate(names)}
        record(f"{what}: worst (|got - sum| - half a bf16 spacing) / bound: " +
               ", ".join(f"{n} {worst[n]:.3f} (onto a base {onto[n]:.3f})" for n in names))


def test_layernorm_rejections(cuda):
    """Shapes the kernels do not take raise before any launch; a valid call follows each."""
    m = _m()
    g = torch.Generator().manual_seed(5)

    def ops(N, C):
        return dev(randn16((N, C), g)), dev(randn16((C,), g)), dev(randn16((C,), g))

    good = ln_case(7, 512, "plain")
    for C in (4104, 68):
        x, w, b = ops(2, C)
        with pytest.raises(RuntimeError):
            m.layernorm_fwd(x, w, b, EPS)
        with pytest.raises(RuntimeError):
            m.add_layernorm_fwd(x, x, w, b, EPS)
        check_ln_forward(good, *run_ln_forward(m, good), f"ln_fwd after the rejected C={C}")
    x, w, b = ops(3, 2056)
    _, mean, rstd = m.layernorm_fwd(x, w, b, EPS)     # the forward takes VPL 5
    with pytest.raises(RuntimeError):
        m.layernorm_bwd(x, x, w, mean, rstd)
    with pytest.raises(RuntimeError):
        m.layernorm_bwd_add(x, x, w, mean, rstd, x, True)
    x, w, b = ops(3, 2048)
    _, mean, rstd = m.layernorm_fwd(x, w, b, EPS)
    dx = m.layernorm_bwd(x, x, w, mean, rstd)[0]
    assert bool(torch.isfinite(dx.float()).all())


# ---------------------------------------------------------------------------------------------
# bias + GELU: references and cases (CPU)
# ---------------------------------------------------------------------------------------------
GK0, GK1 = 0.7978845608028654, 0.044715
X_LIMIT = 8.0
SWEEP_LIMIT = 2.0 ** 40
SWEEP_REL, SWEEP_FLOOR = 2.0 ** -8, 2.0 ** -120
BAND_MIN = 2.0 ** -126   # bf16 subnormal results (below it) are held to the relative rule: they may be flushed
GELU_FWD = [
    (3, 8, "smallest row"),
    (1100, 4096, "F8 % 256 == 0: 2048 blocks, two grid-stride trips, the second ragged"),
    (4200, 1000, "period F8 = 125: 2000 blocks, two trips, the second ragged"),
    (77, 3072, "F8 = 384 is no multiple of 256: period 384, 116 blocks rounded up to 384, most of them idle"),
]
GELU_BWD = [
    (5, 64, "gy = N, one row per y-block"),
    (2049, 64, "gy = 2048, rows_per 2: y-blocks >= 1025 are empty and write zero partials"),
    (8195, 8, "rows_per 5: one full unroll of 4 and a remainder of 1"),
    (77, 3072, "gx = 2 with 128 idle threads in the second x-block"),
]


def gelu_ref(x):
    """tanh-GELU in float64 as x sigma(2u): no cancellation for x << 0."""
    u2 = 2.0 * GK0 * (x + GK1 * x ** 3)
    return x / (1.0 + torch.exp(-u2))


def gelu_grad_ref(x):
    """d/dx of gelu_ref: s + x s (1 - s) 2u', with 1 - s = sigma(-2u) formed on its own."""
    u2 = 2.0 * GK0 * (x + GK1 * x ** 3)
    s, c = 1.0 / (1.0 + torch.exp(-u2)), 1.0 / (1.0 + torch.exp(u2))
    xsc = torch.where((s == 0) | (c == 0), torch.zeros_like(x), x * s * c)
    return s + xsc * (2.0 * GK0 * (1.0 + 3.0 * GK1 * x * x))


def gelu_bias(F, shift=0):
    """Multiples of GB_STEP in [-1.5, 1.5] with a period of 193 columns (89 is coprime to the prime
    193): two columns hold the same bias only at a distance that is a multiple of 193."""
    j = (torch.arange(F, dtype=torch.int64) + shift) * 89 % 193 - 96
    return j.to(F64) * GB_STEP


@functools.lru_cache(maxsize=None)
def gelu_case(N, F, integer_dy=True):
    """x in [-6.5, 6.5] (normal, sd 2.5, clamped), bias in [-1.5, 1.5]: |x + b| <= 8, and the fp32
    sum is exact or not as it falls — the argument is the fp32 sum either way."""
    gen = torch.Generator().manual_seed(3000017 * N + F)
    x = randn16((N, F), gen, 2.5).clamp(-6.5, 6.5)
    b = gelu_bias(F)
    dy = torch.randint(-8, 9, (N, F), generator=gen).to(F64)
    return dict(N=N, F=F, x=x, b=b, dy=dy, base=randn16((F,), gen, 16.0))


def gelu_arg(x, b):
    """The fp32 sum the kernels form, as float64."""
    return (x.to(torch.float32) + b.to(torch.float32)).to(F64)


def gelu_refs(c, b=None):
    a = gelu_arg(c["x"], c["b"] if b is None else b)
    assert float(a.abs().max()) <= X_LIMIT
    d = c["dy"] * gelu_grad_ref(a)
    return dict(y=gelu_ref(a), dx=d, db=d.sum(0), db_abs=d.abs().sum(0))


def check_db(got, c, r, what, base=None):
    s = r["db"] if base is None else r["db"] + base
    bound = db_bound(s, r["db_abs"], c["N"])
    if base is not None:
        bound = bound + U * (base.abs() + r["db_abs"])
    err = (got.cpu().double() - s).abs()
    worst = float((err / bound).max())
    record(f"{what}: worst |db - sum| / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: column {int((err / bound).argmax())} at {worst:.3f} of its bound"


@functools.lru_cache(maxsize=None)
def sweep_patterns():
    """[64, 1024] bf16 holding every 16-bit pattern once, NaN / Inf patterns replaced by +0."""
    bits = (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16)
    perm = torch.randperm(65536, generator=torch.Generator().manual_seed(11))   # patterns spread over the columns
    x = bits[perm].view(BF16).reshape(64, 1024).clone()
    x[~torch.isfinite(x.float())] = 0.0
    return x


def sweep_check(got, v, arg, what):
    """The contract of the module docstring; returns the per-zone counts."""
    got = got.cpu()
    g = got.double()
    a = arg.abs()
    inside, mid = a <= X_LIMIT, (a > X_LIMIT) & (a <= SWEEP_LIMIT)
    small = v.abs() < BAND_MIN
    band_zone, rel_zone = inside & ~small, mid | (inside & small)
    vb = torch.where(band_zone, v, torch.ones_like(v))          # harmless values outside the zone
    want, other, amb = activation_expect(torch.where(band_zone, got, torch.ones_like(got)), vb)
    bad_band = band_zone & (want.view(torch.int16) != got.view(torch.int16))
    tol = SWEEP_REL * v.abs() + SWEEP_FLOOR
    bad_rel = rel_zone & ~(torch.isfinite(g) & ((g - v).abs() <= tol))
    worst = float(torch.where(rel_zone & torch.isfinite(g), (g - v).abs() / tol, torch.zeros_like(v)).max())
    beyond = ~(inside | mid)
    record(f"{what}: {int(band_zone.sum())} band-rule elements ({other} non-nearest, {amb} in the band), "
           f"{int(rel_zone.sum())} relative-rule elements (worst / bound {worst:.3f}), {int(beyond.sum())} beyond "
           f"2^40 of which {int((beyond & ~torch.isfinite(g)).sum())} non-finite")
    for name, bad in (("band", bad_band), ("relative", bad_rel)):
        if bool(bad.any()):
            k = int(bad.reshape(-1).nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} elements break the {name} rule, first at argument "
                                 f"{float(arg.reshape(-1)[k])!r}: got {float(g.reshape(-1)[k])!r}, "
                                 f"float64 {float(v.reshape(-1)[k])!r}")
    return int(band_zone.sum()), int(rel_zone.sum()), int(beyond.sum())


# ---------------------------------------------------------------------------------------------
# bias + GELU: GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F,why", GELU_FWD, ids=[f"{s[0]}x{s[1]}" for s in GELU_FWD])
def test_bias_gelu_forward(cuda, N, F, why):
    c = gelu_case(N, F)
    y = _m().bias_gelu_fwd(dev(c["x"]), dev(c["b"]))
    check_activation(y, gelu_refs(c)["y"], f"bias_gelu_fwd {N}x{F} ({why})")


@pytest.mark.parametrize("N,F,why", GELU_BWD, ids=[f"{s[0]}x{s[1]}" for s in GELU_BWD])
def test_bias_gelu_backward(cuda, N, F, why):
    m, c = _m(), gelu_case(N, F)
    r = gelu_refs(c)
    x, b, dy = dev(c["x"]), dev(c["b"]), dev(c["dy"])
    what = f"bias_gelu_bwd {N}x{F} ({why})"
    dx, db = m.bias_gelu_bwd(dy, x, b)
    check_activation(dx, r["dx"], f"{what} dx")
    check_db(db, c, r, f"{what} db")
    dest = dev(c["base"])
    (dx2,) = m.bias_gelu_bwd(dy, x, b, db_out=dest)
    assert same_bits(dx2, dx)
    check_db(dest, c, r, f"{what} db onto a base", base=c["base"])


@pytest.mark.parametrize("shift", (None, 0), ids=("zero-bias", "bias"))
def test_gelu_every_bf16_pattern(cuda, shift):
    """gelu_sig and gelu_sig_grad (dy = 1) at every bf16 input: the contract of the module docstring."""
    m = _m()
    x = sweep_patterns()
    b = torch.zeros(1024, dtype=F64) if shift is None else gelu_bias(1024, shift)
    arg = gelu_arg(x, b)
    xd, bd = x.cuda(), dev(b)
    y = m.bias_gelu_fwd(xd, bd)
    sweep_check(y, gelu_ref(arg), arg, "gelu_sig over all bf16")
    dx, _ = m.bias_gelu_bwd(torch.ones_like(xd), xd, bd)
    sweep_check(dx, gelu_grad_ref(arg), arg, "gelu_sig_grad over all bf16")


# ---------------------------------------------------------------------------------------------
# embedding: cases and host references (CPU)
# ---------------------------------------------------------------------------------------------
EMB_SEG = 256
EMB_FWD = [(1, 1, 8), (3, 5, 520), (2, 64, 768)]   # smallest; N % 4 != 0 with a c8-loop remainder; general
EMB_VP = 16
# sorted (id, run length) lists; the rows are then scattered by a fixed permutation
PATTERNS = {
    "785a": (5, 157, [(-7, 1), (-3, 2), (-1, 2), (0, 1), (1, 3), (2, 41), (3, 470), (4, 248), (6, 17)]),
    "785b": (5, 157, [(-7, 1), (-3, 2), (-1, 2), (0, 1), (1, 3), (2, 41), (3, 206), (4, 300), (5, 212), (6, 10),
                      (EMB_VP, 3), (EMB_VP + 5, 4)]),
    "768": (3, 256, [(-9, 2), (-2, 1), (0, 100), (1, 153), (2, 1), (3, 200), (5, 55), (7, 256)]),
}


@functools.lru_cache(maxsize=None)
def id_pattern(name):
    """(B, S, idx [B, S] int64): the pattern's runs, rows scattered so that perm is no identity."""
    B, S, runs = PATTERNS[name]
    ids = torch.tensor([t for t, n in runs for _ in range(n)], dtype=torch.int64)
    assert ids.numel() == B * S
    place = torch.randperm(B * S, generator=torch.Generator().manual_seed(B * S))
    idx = torch.empty(B * S, dtype=torch.int64)
    idx[place] = ids
    return B, S, idx.reshape(B, S)


def run_kinds(keys, Vp):
    """The set of piece-rule situations among the runs of valid ids in sorted keys."""
    N = keys.numel()
    k = keys.tolist()
    kinds, a = set(), 0
    if k[0] < 0:
        kinds.add("negative ids")
    if k[-1] >= Vp:
        kinds.add("ids >= Vp")
    while a < N:
        e = a
        while e < N and k[e] == k[a]:
            e += 1
        if 0 <= k[a] < Vp:
            first, last = a // EMB_SEG, (e - 1) // EMB_SEG
            if a % EMB_SEG and last >= first + 2:
                kinds.add("mid-segment through a whole segment into the next")
            if e % EMB_SEG == 0 and e < N:
                kinds.add("ends at a boundary, another id follows")
            if a % EMB_SEG == 0 and a > 0:
                kinds.add("starts at a boundary")
            if a % EMB_SEG == 0 and a > 0 and last > first:
                kinds.add("starts at a boundary and crosses the next")
            if a == EMB_SEG and e == a + 1:
                kinds.add("length 1 at row 256")
            if e == N:
                kinds.add("reaches row N - 1")
            if e == N and N % EMB_SEG == 0:
                kinds.add("ends at N on a boundary")
            if a % EMB_SEG == 0 and e - a == EMB_SEG:
                kinds.add("covers exactly one segment")
        a = e
    return kinds


PATTERN_KINDS = {
    "785a": {"negative ids", "mid-segment through a whole segment into the next",
             "ends at a boundary, another id follows", "starts at a boundary", "reaches row N - 1"},
    "785b": {"negative ids", "ids >= Vp", "ends at a boundary, another id follows", "starts at a boundary",
             "starts at a boundary and crosses the next"},
    "768": {"negative ids", "ends at a boundary, another id follows", "starts at a boundary", "length 1 at row 256",
            "reaches row N - 1", "ends at N on a boundary", "covers exactly one segment"},
}


def sorted_reference(dy, keys, perm, base):
    """embed_bwd_sorted's d(wte) on the host, in its documented order and in fp32 (numpy, one
    rounding per addition, no fma): pieces = runs of equal sorted ids cut at 256-row segments, each
    piece summed from 0 in sorted order; a run inside one segment: piece + existing row -> RNE; a
    crossing run: the partial of its first segment, then the following segments' partials in segment
    order, then + existing row -> RNE.  dy [N, C] float32 of bf16 values, base [Vp, C] bf16."""
    d = dy.numpy().astype(np.float32)
    k, p = keys.tolist(), perm.tolist()
    N, Vp = len(k), base.shape[0]
    out = base.clone()
    a = 0
    while a < N:
        e = a
        while e < N and k[e] == k[a]:
            e += 1
        if 0 <= k[a] < Vp:
            total = None
            lo = a
            while lo < e:
                hi = min(e, (lo // EMB_SEG + 1) * EMB_SEG)
                piece = np.zeros(d.shape[1], np.float32)
                for j in range(lo, hi):
                    piece = piece + d[p[j]]
                total = piece if total is None else total + piece
                lo = hi
            total = total + base[k[a]].to(torch.float32).numpy()
            out[k[a]] = torch.from_numpy(total).to(BF16)
        a = e
    return out


def order_pins(dy, base, keys, perm):
    """Columns 0 and 1 of every run that crosses a segment boundary b are zero but for three rows, so
    that the piece order shows after the bf16 rounding (random sums rarely differ there).  In fp32
    2^24 + 1 = 2^24 (tie to even) and 1 - 2^24 is exact:
        column 0: 2^24, 1, -2^24 at sorted rows b-2, b-1, b: pieces 2^24 | -2^24, sum 0; with rows
                  b-1 and b swapped the pieces are 0 | 1, sum 1
        column 1: the same at b-1, b, b+1: pieces 2^24 | 1 - 2^24, sum 1; summed straight through the
                  run it would be 0"""
    N, k = keys.numel(), keys.tolist()
    a = 0
    while a < N:
        e = a
        while e < N and k[e] == k[a]:
            e += 1
        b = (a // EMB_SEG + 1) * EMB_SEG
        if 0 <= k[a] < base.shape[0] and a + 2 <= b < e - 1:
            dy[perm[a:e], :2] = 0.0
            base[k[a], :2] = 0.0
            for col, first in ((0, b - 2), (1, b - 1)):
                dy[perm[first:first + 3], col] = torch.tensor([2.0 ** 24, 1.0, -2.0 ** 24], dtype=F64)
        a = e


@functools.lru_cache(maxsize=None)
def sorted_case(name, C):
    B, S, idx = id_pattern(name)
    gen = torch.Generator().manual_seed(4000037 * B * S + C)
    dy = randn16((B, S, C), gen)
    base = randn16((EMB_VP, C), gen, 4.0).to(BF16)
    keys, perm = torch.sort(idx.flatten(), stable=True)
    order_pins(dy.view(B * S, C), base, keys, perm)
    want = sorted_reference(dy.reshape(B * S, C).to(torch.float32), keys, perm, base)
    f = dy.to(torch.float32)
    t = torch.zeros(S, C, dtype=torch.float32)
    for bb in range(B):
        t = t + f[bb]
    return dict(B=B, S=S, C=C, idx=idx, dy=dy, base=base, keys=keys, perm=perm, want=want, dwpe=t.to(BF16))


# ---------------------------------------------------------------------------------------------
# embedding: GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,C", EMB_FWD)
def test_embed_forward_exact(cuda, B, S, C):
    """y = RNE(wte[id] + wpe[s]) bit for bit: P > S, ids 0 and Vp - 1 present, all rows distinct."""
    gen = torch.Generator().manual_seed(B * S * C)
    Vp, P = 37, S + 3
    wte, wpe = randn16((Vp, C), gen).to(BF16), randn16((P, C), gen).to(BF16)
    idx = torch.randint(0, Vp, (B, S), generator=gen)
    idx.view(-1)[0], idx.view(-1)[-1] = Vp - 1, 0
    y = _m().embed_fwd(idx.cuda(), wte.cuda(), wpe.cuda())
    want = (wte.float()[idx] + wpe.float()[:S]).to(BF16)
    assert y.shape == (B, S, C)
    check_bits(y.reshape(B * S, C), want.reshape(B * S, C), f"embed_fwd {B}x{S}x{C}")


@pytest.mark.parametrize("B,S,C", [(3, 5, 520), (4, 64, 64)])
def test_embed_backward_atomic_exact(cuda, B, S, C):
    """Integer dy: dwte = RNE(float64 index_add) whatever the atomic order; absent rows +0; ids < 0
    and >= Vp add nothing.  Random dy: dwpe[s] = RNE(fp32 sum over b in order); rows S .. P-1 are +0."""
    m = _m()
    gen = torch.Generator().manual_seed(B * S + C)
    Vp, P, N = 23, S + 4, B * S
    idx = torch.randint(0, Vp - 3, (B, S), generator=gen)       # ids Vp-3 .. Vp-1 never occur
    idx.view(-1)[[1, N // 2]] = torch.tensor([-1, -5])
    idx.view(-1)[[2, N - 1]] = torch.tensor([Vp, Vp + 9])
    dyi = torch.randint(-8, 9, (B, S, C), generator=gen).to(F64)
    dwte, _ = m.embed_bwd(dev(dyi), idx.cuda(), Vp, P)
    flat, ok = idx.flatten(), (idx.flatten() >= 0) & (idx.flatten() < Vp)
    ref = torch.zeros(Vp, C, dtype=F64).index_add_(0, flat[ok], dyi.reshape(N, C)[ok])
    check_bits(dwte, as_bf16(rne(ref)), f"embed_bwd dwte {B}x{S}x{C}")
    assert int((dwte[Vp - 3:].cpu().view(torch.int16) != 0).sum()) == 0, "rows of absent tokens must be +0"
    dyr = randn16((B, S, C), gen)
    _, dwpe = m.embed_bwd(dev(dyr), idx.cuda(), Vp, P)
    t = torch.zeros(S, C, dtype=torch.float32)
    for bb in range(B):
        t = t + dyr[bb].to(torch.float32)
    want = torch.zeros(P, C, dtype=BF16)
    want[:S] = t.to(BF16)
    check_bits(dwpe, want, f"embed_bwd dwpe {B}x{S}x{C}")


@pytest.mark.parametrize("C", (64, 520))
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_embed_backward_sorted_exact(cuda, name, C):
    """embed_bwd_sorted onto a random bf16 base, bit for bit against sorted_reference; untouched rows
    keep the base's bits; dwpe as in the atomic path; two calls give identical bits."""
    m, c = _m(), sorted_case(name, C)
    assert run_kinds(c["keys"], EMB_VP) == PATTERN_KINDS[name]
    dy, keys, perm = dev(c["dy"]), c["keys"].cuda(), c["perm"].cuda()
    P = c["S"] + 2
    slots = [c["base"].cuda(), c["base"].cuda()]
    dwpe = [m.embed_bwd_sorted(dy, keys, perm, s, P) for s in slots]
    check_bits(slots[0], c["want"], f"embed_bwd_sorted {name} C={C}")
    used = set(t for t in c["keys"].tolist() if 0 <= t < EMB_VP)
    idle = [t for t in range(EMB_VP) if t not in used]
    assert idle and same_bits(slots[0].cpu()[idle], c["base"][idle])
    want = torch.zeros(P, C, dtype=BF16)
    want[:c["S"]] = c["dwpe"]
    check_bits(dwpe[0], want, f"embed_bwd_sorted dwpe {name} C={C}")
    assert same_bits(slots[0], slots[1]) and same_bits(dwpe[0], dwpe[1])
