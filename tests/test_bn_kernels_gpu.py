"""Per-channel fp64 and exact checks of the BatchNorm and pooling kernels (batchnorm.hip, pool.hip).

Every entry point of the ResNet path is called straight through the extension and compared, element
by element and channel by channel, with a plain float64 formula on the same bf16 inputs; the tests
build the [G, 2, C] partials themselves.  Tensors are channels_last [N, C, H, W] handled as row-major
[M = N·H·W, C]; every tensor handed to a kernel is a fresh allocation.

Documented behaviour the references state rather than test away: the running variance uses the
unbiased factor M / (M − 1), and 1 at M = 1; the stats-pass forward accumulates d = x − K, K = row 0
of x, so its variance error is relative to Σd², not to Σ(x − mean)².

Error model (u = 2^-24, first order in u).  A correct kernel's output is the float64 value plus
counted fp32 roundings plus one final bf16 rounding.

  fp32 sum of n terms t_i by a chain of at most L additions (serial rows per thread, LDS tree, serial
  partial rows of the finalize, wave butterflies; L is computed from the launch geometry by the
  chain_* functions below, which repeat stats_grid):        |Σ̂ − Σ| ≤ (L + c)·u·Σ|t_i|,
  c = the roundings inside one term.

  stats-pass forward, d = x − K:
    Σd:  c = 1 (d).  md = Σ̂d·(1/M): + 2 →            e_md  = (L + 3)·u·Σ|d| / M
    mean = K + md:                                     e_mean = e_md + u·|mean|
    Σd²: c = 3 (d twice, the product); ·(1/M): + 2; − md²: 2|md|·e_md + u·md²; the subtraction: u·A
                                                       e_var = (L + 6)·u·A + 2|md|·e_md + u·md²,  A = Σd²/M
  forward from tile partials, one level over rows (s_i ± es_i, m2_i ± em_i, n_i), total n:
    S = Σs_i                                           eS = Σes_i + L·u·Σ|s_i|
    mean = S·(1/n)                                     e_mean = eS/n + 2u·|mean|
    d_i = s_i·(1/n_i) − mean                           e_d = es_i/n_i + 2u·|s_i/n_i| + e_mean + u·|d_i|
    term_i = m2_i + n_i·d_i²                           e_t = em_i + 2n_i|d_i|·e_d + 2u·n_i·d_i² + u·term_i
    Q = Σterm_i                                        eQ = Σe_t + L·u·Σterm_i
    the builder's fp32 rounding gives es = u|s|, em = u·m2; with G > 512 the level runs per 256-row
    chunk (L = 8) and again over the chunks; var = Q/M: e_var = eQ/M + u·var
  invstd = rsqrtf(var + eps), 2u allowed for rsqrtf:   e_inv = invstd·(½(e_var + u(var+eps))/(var+eps) + 2u)
  sc = γ·invstd:                                       e_sc = |γ|·e_inv + u·|sc|
  v = x·sc + (β − mean·sc): the error of sc enters through (x − mean)·sc,
    e_v = |x − mean|·e_sc + |sc|·e_mean + u·|mean·sc| + u·(|β| + |mean·sc|) + u·|x·sc| + u·(|x·sc| + |sh|)
    (+ u·|v + res| per residual add; the pair adds both sides' e_v)
  bf16 output:                                         |got − ref| ≤ 2^-8·|ref| + (1 + 2^-8)·e_v
  running statistics new = (1−m)·old + m·[unb]·stat:   5u·(|(1−m)·old| + |m·unb·stat|) + m·unb·e_stat

  backward with mean and invstd GIVEN (the fp32 values the kernel receives), g = dy·mask exact, xc = x − μ:
    s1 = Σg: c = 0                                     e_s1 = L·u·Σ|g|   (0 where the sums are integers < 2^24)
    s2 = Σg·xc: c = 2 (xc, the product)                e_s2 = (L + 2)·u·Σ|g·xc|
    dγ = s2·invstd                                     e_dγ = invstd·e_s2 + u·|dγ|
    k = γ·invstd; k1 = k·s1·(1/M): 4 roundings         e_k1 = |k|·e_s1/M + 4u·|k1|
    k2 = k·invstd·dγ·(1/M): 5 roundings                e_k2 = |k·invstd|·e_dγ/M + 5u·|k2|
    dx = k·g − k1 − k2·xc                              e_dx = 2u|k·g| + e_k1 + e_k2·|xc| + 2u|k2·xc|
                                                              + 2u(|k·g| + |k1| + |k2·xc|)
    accumulation into a given gradient:                + u·|old + new|

A flipped ReLU mask is an O(|dy|) error, not a rounding: before a backward that recomputes the mask
from x, dy is set to 0 wherever the float64 pre-activation lies within e_v of zero (asserted to be
under 0.1 % of the elements), and nothing is excluded after the fact.  When y or a mask is passed the
reference mask is the kernel forward's own output, which is validated separately.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = 2.0 ** -8
BF16 = torch.bfloat16
F64 = torch.float64
L_MAX = 40  # every chain length used by a bound is asserted to stay under this


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def f32(x):
    """x rounded to float32, as a Python float: what a kernel receives for a scalar argument."""
    return float(np.float32(x))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _worst(err, bound):
    """max err / bound (a bound of 0 admits only err = 0)."""
    return float((err / bound.clamp_min(1e-300)).max())


class Report:
    """Collects max(err / bound) per output and fails once, naming every output over its bound."""

    def __init__(self, what):
        self.what, self.rows = what, []

    def add(self, name, got, ref, bound):
        assert got.shape == ref.shape, f"{self.what}: {name} shape {tuple(got.shape)} vs {tuple(ref.shape)}"
        assert bool(torch.isfinite(got).all()), f"{self.what}: {name} is not finite"
        self.rows.append((name, _worst((got.double() - ref).abs(), bound.expand_as(ref))))

    def exact(self, name, ok):
        self.rows.append((name, 0.0 if ok else math.inf))

    def check(self):
        print(f"bn-ratio | {self.what} | " + "  ".join(f"{n} {r:.3g}" for n, r in self.rows))
        bad = [(n, r) for n, r in self.rows if not r <= 1.0]
        assert not bad, f"{self.what}: err / bound over 1 for {bad}"


def nhwc(rows, N, H, W):
    """[M, C] rows → the channels_last [N, C, H, W] view of the same memory."""
    return rows.reshape(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def rows_of(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def unpack_mask(mask, M, C):
    """bit j of byte i → element 8i + j, as a bool [M, C]."""
    b = (mask.to(torch.int32)[:, None] >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return b.reshape(M, C).bool()


# ---------------------------------------------------------------------------------------------
# launch geometry → addition chain lengths (the formulas of pick_tx / stats_grid / the finalizes)
# ---------------------------------------------------------------------------------------------
def stats_grid(M, C):
    c8 = C // 8
    tx = 32 if c8 >= 32 else 16 if c8 >= 16 else 8
    gx = (c8 + tx - 1) // tx
    gy = max(1, min((2048 + gx - 1) // gx, (M + 63) // 64))
    return tx, gx, gy, (M + gy - 1) // gy


def chain_rows(G, merged):
    """block_sum_partials over G partial rows: serial rows per lane + 6 butterflies + 3 wave totals;
    with G > 512 and a merge buffer, bn_sum_rows first (6 butterflies + 2)."""
    L = 0
    if merged and G > 512:
        G, L = (G + 255) // 256, 8
    return L + (G + 255) // 256 + 9


def chain_stats(M, C, merged):
    """stats kernel (serial rows per thread + LDS tree over TY) and its finalize."""
    tx, _, gy, rpg = stats_grid(M, C)
    ty = 256 // tx
    return (rpg + ty - 1) // ty + int(math.log2(ty)) + chain_rows(gy, merged)


def chain_tiles(G):
    """bn_finalize_tiles_kernel: 3 additions per trip of 1024 rows, 6 butterflies, 2 for the wave totals."""
    return 3 * ((G + 1023) // 1024) + 8


# ---------------------------------------------------------------------------------------------
# references (float64, plain formulas; validated on the CPU in test_bn_kernels_cpu.py)
# ---------------------------------------------------------------------------------------------
def bn_stats_ref(x):
    """per-channel mean and biased variance of x [M, C] (float64)."""
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def bn_fwd_ref(x, w, b, eps, relu, add=None):
    """y = act(x̂·γ + β [+ add]) with invstd = (var + eps)^-1/2; float64 [M, C] in, a dict out."""
    mean, var = bn_stats_ref(x)
    inv = (var + eps) ** -0.5
    pre = (x - mean) * inv * w + b
    if add is not None:
        pre = pre + add
    return dict(mean=mean, var=var, invstd=inv, pre=pre, y=pre.clamp_min(0.0) if relu else pre)


def running_ref(rm, rv, mean, var, M, mom):
    """momentum update with the unbiased factor M / (M − 1); at M = 1 the factor is 1 (documented)."""
    unb = M / (M - 1.0) if M > 1 else 1.0
    return (1.0 - mom) * rm + mom * mean, (1.0 - mom) * rv + mom * unb * var


def bn_bwd_ref(g, x, mean, invstd, w, M=None):
    """g = dy·mask, mean and invstd given.  dβ = Σg, dγ = invstd·Σg(x−μ),
    dx = γ·invstd·(g − dβ/M − x̂·dγ/M), dres = g.  M defaults to the rows of x."""
    M = x.shape[0] if M is None else M
    xc = x - mean
    db = g.sum(0)
    dg = invstd * (g * xc).sum(0)
    return w * invstd * (g - db / M - xc * invstd * dg / M), dg, db


def tile_partials(x, t, dtype=torch.float32):
    """[G, 2, C] fp32: row i = (Σv, Σ(v − mean_i)²) over rows [i·t, min((i+1)·t, M)) of x [M, C],
    computed in float64 and then rounded (dtype float64: left unrounded, for the CPU self-checks)."""
    M, C = x.shape
    G = (M + t - 1) // t
    xp = torch.zeros(G * t, C, dtype=F64, device=x.device)
    xp[:M] = x
    xp = xp.view(G, t, C)
    n = tile_counts(M, t, x.device)
    live = (torch.arange(t, device=x.device)[None, :] < n[:, None])[..., None]
    s = (xp * live).sum(1)
    m2 = (((xp - (s / n[:, None])[:, None, :]) ** 2) * live).sum(1)
    return torch.stack([s, m2], 1).to(dtype)


def tile_counts(M, t, dev):
    G = (M + t - 1) // t
    n = torch.full((G,), float(t), dtype=F64, device=dev)
    n[-1] = M - (G - 1) * t
    return n


def merge_level(s, m2, n, es=None, em=None, L=0):
    """The documented merge of partial rows (s_i, m2_i, n_i) → (S, Q, eS, eQ):
    S = Σs_i, Q = Σ(m2_i + n_i·(s_i/n_i − S/n)²), with the first-order error bounds of the header."""
    es = torch.zeros_like(s) if es is None else es
    em = torch.zeros_like(m2) if em is None else em
    nt, nn = n.sum(), n[:, None]
    S = s.sum(0)
    eS = es.sum(0) + L * U * s.abs().sum(0)
    mean = S / nt
    e_mean = eS / nt + 2 * U * mean.abs()
    d = s / nn - mean
    e_d = es / nn + 2 * U * (s / nn).abs() + e_mean + U * d.abs()
    term = m2 + nn * d * d
    e_t = em + 2 * nn * d.abs() * e_d + 2 * U * nn * d * d + U * term
    return S, term.sum(0), eS, e_t.sum(0) + L * U * term.sum(0)


def tiles_stats(part, t, M):
    """mean, var and their bounds as bn_finalize_tiles (after bn_merge_tiles when G > 512) can give
    them from fp32 partials; also the total chain length."""
    s, m2 = part[:, 0].double(), part[:, 1].double()
    n = tile_counts(M, t, part.device)
    es, em = U * s.abs(), U * m2
    G, L = s.shape[0], 0
    if G > 512:
        out = [merge_level(s[i:i + 256], m2[i:i + 256], n[i:i + 256], es[i:i + 256], em[i:i + 256], 8)
               for i in range(0, G, 256)]
        s, m2, es, em = (torch.stack([o[k] for o in out]) for k in range(4))
        n = torch.stack([n[i:i + 256].sum() for i in range(0, G, 256)])
        G, L = s.shape[0], 8
    S, Q, eS, eQ = merge_level(s, m2, n, es, em, chain_tiles(G))
    mean, var = S / M, Q / M
    return mean, var, eS / M + 2 * U * mean.abs(), eQ / M + U * var, L + chain_tiles(G)


def pool_windows(a, pad):
    """the nine stride-2 window slices [N, OH, OW, C] of a [N, H, W, C], in (kh, kw) scan order."""
    N, H, W, C = a.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ap = torch.full((N, H + 2, W + 2, C), pad, dtype=a.dtype, device=a.device)
    ap[:, 1:H + 1, 1:W + 1] = a
    return [ap[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] for kh in range(3) for kw in range(3)]


def pool_fwd_ref(a):
    """3×3 / stride 2 / pad 1 max of a [N, H, W, C]; among equal maxima the first in scan order."""
    wins = pool_windows(a, -math.inf)
    best = torch.full_like(wins[0], -math.inf)
    arg = torch.zeros(best.shape, dtype=torch.uint8, device=a.device)
    for p, v in enumerate(wins):
        up = v > best
        best = torch.where(up, v, best)
        arg = torch.where(up, torch.full_like(arg, p), arg)
    return best, arg


def pool_gather(a, arg):
    """a at the window positions arg (NaN where a position lies outside the image)."""
    out = torch.full(arg.shape, math.nan, dtype=a.dtype, device=a.device)
    for p, v in enumerate(pool_windows(a, math.nan)):
        out = torch.where(arg == p, v, out)
    return out


def pool_scatter(dy, arg, H, W):
    """the max-pool backward: every dy added at its window's chosen position; [N, H, W, C]."""
    N, OH, OW, C = dy.shape
    dxp = torch.zeros(N, H + 2, W + 2, C, dtype=dy.dtype, device=dy.device)
    for p in range(9):
        kh, kw = divmod(p, 3)
        dxp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += torch.where(arg == p, dy, torch.zeros_like(dy))
    return dxp[:, 1:H + 1, 1:W + 1]


# ---------------------------------------------------------------------------------------------
# bounds (the header's formulas)
# ---------------------------------------------------------------------------------------------
def fwd_stats_bound(x, L):
    """e_mean, e_var of the stats-pass forward over x [M, C] float64."""
    M = x.shape[0]
    d = x - x[0]
    md = d.mean(0)
    e_md = (L + 3) * U * d.abs().sum(0) / M
    e_mean = e_md + U * x.mean(0).abs()
    e_var = (L + 6) * U * (d * d).sum(0) / M + 2 * md.abs() * e_md + U * md * md
    return e_mean, e_var


def invstd_bound(var, eps, e_var):
    return (var + eps) ** -0.5 * (0.5 * (e_var + U * (var + eps)) / (var + eps) + 2 * U)


def preact_bound(x, mean, inv, w, b, e_mean, e_inv):
    """e_v of v = x·sc + sh for sc = γ·invstd, sh = β − mean·sc."""
    sc = w * inv
    e_sc = w.abs() * e_inv + U * sc.abs()
    msc = (mean * sc).abs()
    return ((x - mean).abs() * e_sc + sc.abs() * e_mean + U * msc + U * (b.abs() + msc) + U * (x * sc).abs()
            + U * ((x * sc).abs() + b.abs() + msc))


def out_bound(ref, e):
    return BF * ref.abs() + (1 + BF) * e


def running_bound(old, stat, e_stat, mom, unb):
    return 5 * U * (((1 - mom) * old).abs() + (mom * unb * stat).abs()) + mom * unb * e_stat


def bwd_sums(g, xc, L, exact_s1=True):
    """(s1, s2, e_s1, e_s2) of Σg and Σg·xc over the rows; integer g with |Σ| < 2^24 sums exactly."""
    s1, s2 = g.sum(0), (g * xc).sum(0)
    e_s1 = torch.zeros_like(s1) if exact_s1 else L * U * g.abs().sum(0)
    return s1, s2, e_s1, (L + 2) * U * (g * xc).abs().sum(0)


def bwd_bound(s1, s2, e_s1, e_s2, g, xc, inv, w, M):
    """(e_dx [rows, C], e_dγ, e_dβ) from the sums' bounds; g and xc are the rows dx is written for."""
    dg = s2 * inv
    e_dg = inv * e_s2 + U * dg.abs()
    k = w * inv
    k1, k2 = k * s1 / M, k * inv * dg / M
    e_k1 = k.abs() * e_s1 / M + 4 * U * k1.abs()
    e_k2 = (k * inv).abs() * e_dg / M + 5 * U * k2.abs()
    t0, t2 = (k * g).abs(), (k2 * xc).abs()
    e_dx = 2 * U * t0 + e_k1 + e_k2 * xc.abs() + 2 * U * t2 + 2 * U * (t0 + k1.abs() + t2)
    return e_dx, e_dg, e_s1


# ---------------------------------------------------------------------------------------------
# inputs (built on the CPU from a seed, so the CPU file sees exactly what the GPU tests use)
# ---------------------------------------------------------------------------------------------
KINDS = ("normal", "bigmean", "outlier", "const", "gneg", "gzero")
EPS, MOM = f32(1e-5), f32(0.1)


def bn_inputs(M, C, seed, dev="cpu"):
    """x, res, dy (bf16 [M, C]); w, b, rm, rv (fp32 [C]).  Channel c is of kind KINDS[c % 6]:
    ordinary N(μ_c, σ_c); 64 + 0.5k, k ∈ [−4, 4]; row 0 an 8σ outlier; constant; γ < 0; γ = 0.
    dy is integer-valued in [−4, 4]; |β| ≥ 0.05."""
    g = torch.Generator().manual_seed(seed)
    kind = torch.arange(C) % 6
    mu = torch.rand(C, generator=g) * 6 - 3
    sig = torch.rand(C, generator=g) * 1.5 + 0.5
    x = mu + sig * torch.randn(M, C, generator=g)
    big = 64 + 0.5 * torch.randint(-4, 5, (M, C), generator=g)
    x = torch.where(kind == 1, big, x)
    x[0] = torch.where(kind == 2, mu + 8 * sig, x[0])
    x = torch.where(kind == 3, mu.expand(M, C), x)
    w = torch.rand(C, generator=g) + 0.5
    w = torch.where(kind == 4, -w, w)
    w = torch.where(kind == 5, torch.zeros_like(w), w)
    b = 0.5 * torch.randn(C, generator=g)
    b = torch.where(b < 0, b - 0.05, b + 0.05)
    res = torch.randn(M, C, generator=g)
    dy = torch.randint(-4, 5, (M, C), generator=g).float()
    rm = 0.1 * torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    d = dict(x=x.bfloat16(), res=res.bfloat16(), dy=dy.bfloat16(), w=w, b=b, rm=rm, rv=rv)
    return {k: v.to(dev) for k, v in d.items()}


def ramp_inputs(M, C, seed, dev="cpu"):
    """a per-channel ramp along the rows plus noise: the between-tile term n_i(mean_i − mean)² is most
    of the variance."""
    g = torch.Generator().manual_seed(seed)
    slope = (torch.rand(C, generator=g) * 4 + 2) * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    x = slope * (torch.arange(M)[:, None] / max(M, 1) - 0.5) + 0.1 * torch.randn(M, C, generator=g) \
        + torch.randn(C, generator=g)
    d = bn_inputs(M, C, seed + 1)
    d["x"] = x.bfloat16()
    return {k: v.to(dev) for k, v in d.items()}


def near_zero(x, mean, inv, w, b):
    """bool [M, C]: the float64 pre-activation from the GIVEN fp32 mean and invstd lies within the
    fp32 bound of zero (only the roundings of sc, sh and the multiply-add: mean and invstd are inputs)."""
    z = torch.zeros_like(mean)
    pre = (x - mean) * inv * w + b
    return pre.abs() <= preact_bound(x, mean, inv, w, b, z, z)


def zero_near(dy, nz):
    """dy with the near-zero elements cleared; the share cleared must be under 0.1 %."""
    share = float(nz.double().mean())
    assert share < 1e-3, f"{share:.2%} of the pre-activations lie within the fp32 bound of zero"
    return torch.where(nz, torch.zeros_like(dy), dy)


# ---------------------------------------------------------------------------------------------
# 1. stats-pass forward and backward
# ---------------------------------------------------------------------------------------------
def _fresh(t):
    return t.clone()


def check_fwd(rep, tag, x, w, b, eps, relu, y, mean, invstd, e_mean, e_var, add=None, e_add=None):
    """y, mean, invstd against float64 of x; returns the reference dict and e_v."""
    ref = bn_fwd_ref(x, w, b, eps, relu, add)
    e_inv = invstd_bound(ref["var"], eps, e_var)
    e_v = preact_bound(x, ref["mean"], ref["invstd"], w, b, e_mean, e_inv)
    if add is not None:
        e_v = e_v + e_add + U * ref["pre"].abs()
    rep.add(tag + "mean", mean, ref["mean"], e_mean)
    rep.add(tag + "invstd", invstd, ref["invstd"], e_inv)
    rep.add(tag + "y", y, ref["y"], out_bound(ref["y"], e_v))
    ref["e_var"], ref["e_mean"] = e_var, e_mean
    return ref, e_v


def check_running(rep, tag, rm, rv, rm0, rv0, ref, M, mom):
    unb = M / (M - 1.0) if M > 1 else 1.0
    rm_ref, rv_ref = running_ref(rm0, rv0, ref["mean"], ref["var"], M, mom)
    rep.add(tag + "rmean", rm, rm_ref, running_bound(rm0, ref["mean"], ref["e_mean"], mom, 1.0))
    rep.add(tag + "rvar", rv, rv_ref, running_bound(rv0, ref["var"], ref["e_var"], mom, unb))


def check_bwd(rep, tag, out, g, x, mean, invstd, w, L, want_dres, dw0=None, db0=None, into=None, sums=None):
    """[dx, dres, dw, db] of bn_act_bwd / bn_act_bwd_part against bn_bwd_ref with the given fp32 mean
    and invstd.  g = dy·mask (float64).  into = (dw, db) tensors that were prefilled with dw0, db0."""
    M = x.shape[0]
    mu, inv = mean.double(), invstd.double()
    xc = x - mu
    s1, s2, e_s1, e_s2 = bwd_sums(g, xc, L) if sums is None else sums
    dx_ref, dg_ref, db_ref = bn_bwd_ref(g, x, mu, inv, w)
    e_dx, e_dg, e_db = bwd_bound(s1, s2, e_s1, e_s2, g, xc, inv, w, M)
    dx, dres, dw, db = out
    rep.add(tag + "dx", rows_of(dx), dx_ref, out_bound(dx_ref, e_dx))
    if want_dres:
        # dy or +0 bit for bit (dy·0 in the reference's g is −0 for a negative dy)
        rep.exact(tag + "dres", same_bits(rows_of(dres), torch.where(g != 0, g, torch.zeros_like(g)).bfloat16()))
    else:
        assert dres is None
    if into is not None:
        assert dw is None and db is None, "gradients accumulated in place are not returned"
        dw, db = into
        dg_ref, db_ref = dw0 + dg_ref, db0 + db_ref
        e_dg, e_db = e_dg + U * dg_ref.abs(), e_db + U * db_ref.abs()
    rep.add(tag + "dgamma", dw, dg_ref, e_dg)
    rep.add(tag + "dbeta", db, db_ref, e_db)
    return dw, db


def run_stats_case(m, cuda, N, C, H, W, seed, modes):
    """modes: (relu, residual) pairs.  Forward with and without running statistics, backward from y,
    from the mask, recomputed, with and without dres, accumulated and returned."""
    M = N * H * W
    d = bn_inputs(M, C, seed, cuda)
    x64, w64, b64 = d["x"].double(), d["w"].double(), d["b"].double()
    Lf, Lb = chain_stats(M, C, False), chain_stats(M, C, True)
    assert max(Lf, Lb) <= L_MAX
    e_mean, e_var = fwd_stats_bound(x64, Lf)
    rep = Report(f"stats C {C} M {M} (L fwd {Lf}, bwd {Lb})")
    for relu, use_res in modes:
        tag = f"[relu{int(relu)} res{int(use_res)}] "
        xs = nhwc(_fresh(d["x"]), N, H, W)
        res = nhwc(_fresh(d["res"]), N, H, W) if use_res else None
        give_running = relu != use_res
        rm, rv = (_fresh(d["rm"]), _fresh(d["rv"])) if give_running else (None, None)
        y, mean, invstd, mask = m.bn_act_fwd(xs, res, _fresh(d["w"]), _fresh(d["b"]), rm, rv, EPS, MOM, relu)
        add = d["res"].double() if use_res else None
        ref, _ = check_fwd(rep, tag, x64, w64, b64, EPS, relu, rows_of(y), mean, invstd, e_mean, e_var, add,
                           0.0 if use_res else None)
        if give_running:
            check_running(rep, tag, rm, rv, d["rm"].double(), d["rv"].double(), ref, M, MOM)
        assert (mask is not None) == (relu and use_res)
        ypos = rows_of(y) > 0
        if mask is not None:
            rep.exact(tag + "mask", torch.equal(unpack_mask(mask, M, C), ypos))
        # backward
        dy = d["dy"]
        runs = []  # (label, y argument, g)
        if relu and not use_res:
            nz = near_zero(x64, mean.double(), invstd.double(), w64, b64)
            dy = zero_near(dy, nz)
            pre = (x64 - mean.double()) * invstd.double() * w64 + b64
            runs.append(("recomputed ", None, dy.double() * (pre > 0)))
            runs.append(("from y ", y, dy.double() * ypos))
        elif relu:
            runs.append(("from y ", y, dy.double() * ypos))
            runs.append(("from mask ", mask, dy.double() * ypos))
        else:
            runs.append(("", None, dy.double()))
            runs.append(("again ", None, dy.double()))
        for i, (label, yarg, g) in enumerate(runs):
            assert float(g.abs().sum(0).max()) < 2 ** 24
            into = None
            dw0, db0 = d["rm"].double() + 3.0, d["rv"].double() - 2.0
            if i == 1:
                into = (dw0.float(), db0.float())
                dw0, db0 = into[0].double(), into[1].double()
            want_dres = use_res if i == 0 else (use_res and relu)  # relu off: once with dres, once without
            out = m.bn_act_bwd(nhwc(_fresh(dy), N, H, W), yarg, xs, mean, invstd, _fresh(d["w"]), _fresh(d["b"]),
                               relu, want_dres, *(into if into else (None, None)))
            _, db = check_bwd(rep, tag + label, out, g, x64, mean, invstd, w64, Lb, want_dres, dw0, db0, into)
            if into is None:
                rep.exact(tag + label + "dbeta exact", torch.equal(db.double(), g.sum(0)))
    rep.check()


ALL_MODES = [(False, False), (True, False), (False, True), (True, True)]
STATS_C, STATS_M = [8, 24, 64, 136, 320, 2048], [1, 63, 64, 65, 200]
LARGE = [((2, 64, 260, 260), [(True, False)]),   # hoisted apply, second trip; gy = 2048: bn_sum_rows, 8 full chunks
         ((1, 24, 600, 600), [(True, True)]),    # non-hoisted apply, second trip
         ((1, 8, 150, 220), [(False, False)])]   # gy = 516: bn_sum_rows with a ragged last chunk


def stats_seed(C, M):
    return 1000 * C + M


def stem_seed(N, C, H, W):
    return 7 * C + 13 * H + W + N


@pytest.mark.parametrize("M", STATS_M)
@pytest.mark.parametrize("C", STATS_C)
def test_bn_act_stats_pass(cuda, C, M):
    """C 8: TX 8 with one live lane; 24: non-hoisted apply; 64: TX 8, all lanes; 136: TX 16, a second
    block with one live lane; 320: TX 32, a second block with 8 live lanes; 2048: TX 32, gx = 8."""
    tx, gx, _, _ = stats_grid(M, C)
    assert (tx, gx) == {8: (8, 1), 24: (8, 1), 64: (8, 1), 136: (16, 2), 320: (32, 2), 2048: (32, 8)}[C]
    run_stats_case(_m(), cuda, 1, C, 1, M, stats_seed(C, M), ALL_MODES)


@pytest.mark.parametrize("shape,modes", LARGE, ids=["2x64x260x260", "1x24x600x600", "1x8x150x220"])
def test_bn_act_stats_pass_large(cuda, shape, modes):
    N, C, H, W = shape
    M = N * H * W
    gy = stats_grid(M, C)[2]
    if C == 8:
        assert gy == 516
    else:
        assert gy == 2048 and M * C // 8 > 4096 * 256  # the apply loops take a second trip
    run_stats_case(_m(), cuda, N, C, H, W, stats_seed(C, M), modes)


# ---------------------------------------------------------------------------------------------
# 2. the recomputed mask is the forward's mask
# ---------------------------------------------------------------------------------------------
def quantised_inputs(M, C, seed, dev):
    """x on a 0.5 grid in [−3, 3] (few distinct values per channel, window ties), mixed-sign γ,
    integer dy."""
    g = torch.Generator().manual_seed(seed)
    x = (0.5 * torch.randint(-6, 7, (M, C), generator=g)).bfloat16()
    w = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    b = 0.3 * torch.randn(C, generator=g)
    dy = torch.randint(-4, 5, (M, C), generator=g).bfloat16()
    return x.to(dev), w.to(dev), b.to(dev), dy.to(dev)


def beta_for_zero(xstar, mean, invstd, w):
    """β (fp32) that puts x*·sc + sh within a few ulps of zero: β = (mean − x*)·sc, moved by
    j ∈ {−2, …, 2} ulps, j varying along the channels."""
    sc = w * invstd
    b = mean * sc - xstar.float() * sc
    j = torch.arange(b.numel(), device=b.device) % 5 - 2
    for step in (1, 2):
        b = torch.where(j >= step, torch.nextafter(b, torch.full_like(b, math.inf)), b)
        b = torch.where(j <= -step, torch.nextafter(b, torch.full_like(b, -math.inf)), b)
    # x* = mean = 0 gives β = 0: left there (denormal steps away from it, v > 0 would round to a bf16 zero)
    return torch.where(b.abs() < 1e-30, torch.zeros_like(b), b)


@pytest.mark.parametrize("C,M", [(64, 777), (24, 500), (320, 130)])
def test_recomputed_mask_is_forward_mask(cuda, C, M):
    """bn_act_bwd with y = None (mask recomputed from x through affine8 / preact) and with the forward's
    y agree bit for bit when a frequent input value sits within a few ulps of the ReLU's zero."""
    m = _m()
    x, w, b, dy = quantised_inputs(M, C, 5 + C, cuda)
    xs = nhwc(x, 1, 1, M)
    _, mean, invstd, _ = m.bn_act_fwd(xs, None, w, b, None, None, EPS, MOM, False)
    xstar = x[1]
    b0 = beta_for_zero(xstar, mean, invstd, w)
    y, mean2, invstd2, _ = m.bn_act_fwd(xs, None, w, b0, None, None, EPS, MOM, True)
    assert same_bits(mean2, mean) and same_bits(invstd2, invstd)
    on = ((rows_of(y) > 0) & (x == xstar)).any(0)  # per channel: is x* on the positive side?
    assert 0 < int(on.sum()) < C, "x* must fall on both sides of zero across the channels"
    sc = w.double() * invstd.double()
    pre = (xstar.double() - mean.double()) * sc + b0.double()
    # (1e-30: a channel with x* = mean = 0 has β a few denormal steps from 0)
    assert bool((pre.abs() <= 64 * U * ((xstar.double() * sc).abs() + (mean.double() * sc).abs()) + 1e-30).all())
    assert float((x == xstar).double().mean()) > 0.03  # a frequent value
    a = m.bn_act_bwd(nhwc(_fresh(dy), 1, 1, M), None, xs, mean, invstd, w, b0, True, False, None, None)
    c = m.bn_act_bwd(nhwc(_fresh(dy), 1, 1, M), y, xs, mean, invstd, w, b0, True, False, None, None)
    for name, p, q in zip(("dx", "dres", "dgamma", "dbeta"), a, c):
        if name != "dres":
            assert same_bits(p, q), f"{name}: the recomputed mask differs from the forward's"


# ---------------------------------------------------------------------------------------------
# 3. forward from tile partials
# ---------------------------------------------------------------------------------------------
def tiles_M(G, t):
    """G tiles of t rows with a ragged last tile."""
    return (G - 1) * t + (1 if G % 2 else t - 1)


@pytest.mark.parametrize("t", [4, 7])
@pytest.mark.parametrize("G", [1, 5, 512, 513, 600, 1100])
def test_bn_act_fwd_tiles(cuda, G, t):
    """G 512: the last unmerged count; 513: merged, the last chunk holds one row; 600: a ragged chunk;
    1100: five chunks.  mean, invstd, y, mask and running statistics against float64 of x itself."""
    m = _m()
    C, M = 16, tiles_M(G, t)
    d = ramp_inputs(M, C, 31 * G + t, cuda)
    x64, w64, b64 = d["x"].double(), d["w"].double(), d["b"].double()
    part = tile_partials(x64, t)
    assert part.shape == (G, 2, C)
    mean_t, var_t, e_mean, e_var, L = tiles_stats(part, t, M)
    assert L <= L_MAX
    mean64, var64 = bn_stats_ref(x64)
    n = tile_counts(M, t, cuda)[:, None]
    between = (n * (part[:, 0].double() / n - mean64) ** 2).sum(0) / M
    if G > 1:
        assert float((between / var64).min()) > 0.5  # the between-tile term is most of the variance
    rep = Report(f"tiles G {G} t {t} M {M} (L {L})")
    for relu, use_res in ((True, True), (False, False)):
        tag = f"[relu{int(relu)} res{int(use_res)}] "
        xs = nhwc(_fresh(d["x"]), 1, 1, M)
        res = nhwc(_fresh(d["res"]), 1, 1, M) if use_res else None
        rm, rv = (_fresh(d["rm"]), _fresh(d["rv"])) if use_res else (None, None)
        y, mean, invstd, mask = m.bn_act_fwd_tiles(xs, _fresh(part), t, res, _fresh(d["w"]), _fresh(d["b"]), rm, rv,
                                                   EPS, MOM, relu)
        ref, _ = check_fwd(rep, tag, x64, w64, b64, EPS, relu, rows_of(y), mean, invstd, e_mean, e_var,
                           d["res"].double() if use_res else None, 0.0 if use_res else None)
        if use_res:
            check_running(rep, tag, rm, rv, d["rm"].double(), d["rv"].double(), ref, M, MOM)
            rep.exact(tag + "mask", torch.equal(unpack_mask(mask, M, C), rows_of(y) > 0))
        else:
            assert mask is None
    rep.check()


def test_bn_act_fwd_tiles_rejects_wrong_stats(cuda):
    m = _m()
    C, t, M = 16, 4, 19
    d = ramp_inputs(M, C, 3, cuda)
    part = tile_partials(d["x"].double(), t)
    xs = nhwc(d["x"], 1, 1, M)
    for bad in (part[:-1].contiguous(), part[:, :1].contiguous(), part[:, :, :8].contiguous(),
                torch.cat([part, part[:1]])):
        with pytest.raises(RuntimeError):
            m.bn_act_fwd_tiles(xs, bad, t, None, d["w"], d["b"], None, None, EPS, MOM, False)
    with pytest.raises(RuntimeError):
        m.bn_act_fwd_tiles(xs, part, t + 1, None, d["w"], d["b"], None, None, EPS, MOM, False)


# ---------------------------------------------------------------------------------------------
# 4. backward from partials
# ---------------------------------------------------------------------------------------------
def group_sizes(G):
    """row groups of unequal size: 1 + (i mod 5) rows."""
    return 1 + torch.arange(G) % 5


def bwd_partials(g, xc, sizes):
    """[G, 2, C] fp32 (Σg, Σg·xc) over consecutive row groups, float64 then rounded."""
    G = sizes.numel()
    gid = torch.repeat_interleave(torch.arange(G, device=g.device), sizes.to(g.device))
    z = torch.zeros(G, g.shape[1], dtype=F64, device=g.device)
    return torch.stack([z.index_add(0, gid, g), z.index_add(0, gid, g * xc)], 1).float()


@pytest.mark.parametrize("G", [1, 300, 512, 513, 700])
def test_bn_act_bwd_part(cuda, G):
    """bn_act_bwd_part from synthetic (Σg, Σg(x−μ)) partials meets the bounds of bn_act_bwd, and the
    two agree on dγ and dβ within the sum of their fp32 bounds."""
    m = _m()
    C = 24
    sizes = group_sizes(G)
    M = int(sizes.sum())
    d = bn_inputs(M, C, 400 + G, cuda)
    x64, w64 = d["x"].double(), d["w"].double()
    xs, res = nhwc(_fresh(d["x"]), 1, 1, M), nhwc(_fresh(d["res"]), 1, 1, M)
    y, mean, invstd, mask = m.bn_act_fwd(xs, res, _fresh(d["w"]), _fresh(d["b"]), None, None, EPS, MOM, True)
    g = d["dy"].double() * (rows_of(y) > 0)
    xc = x64 - mean.double()
    part = bwd_partials(g, xc, sizes)
    Lp, Lb = chain_rows(G, True), chain_stats(M, C, True)
    assert max(Lp, Lb) <= L_MAX
    p1, p2 = part[:, 0].double(), part[:, 1].double()
    # the partial rows are fp32 roundings of float64 sums (u each) added by a chain of Lp
    sums = (g.sum(0), (g * xc).sum(0), torch.zeros(C, dtype=F64, device=cuda),
            (Lp + 1) * U * p2.abs().sum(0))
    assert torch.equal(p1.sum(0), sums[0])  # integer partial rows: exact in fp32
    rep = Report(f"bwd_part G {G} M {M} (L part {Lp}, stats {Lb})")
    dw0, db0 = d["rm"].double() + 3.0, d["rv"].double() - 2.0
    into = (dw0.float(), db0.float())
    out = m.bn_act_bwd_part(_fresh(part), nhwc(_fresh(d["dy"]), 1, 1, M), mask, xs, mean, invstd, _fresh(d["w"]),
                            _fresh(d["b"]), True, True, None, None)
    dw_p, db_p = check_bwd(rep, "[part] ", out, g, x64, mean, invstd, w64, Lp, True, sums=sums)
    out = m.bn_act_bwd_part(_fresh(part), nhwc(_fresh(d["dy"]), 1, 1, M), y, xs, mean, invstd, _fresh(d["w"]),
                            _fresh(d["b"]), True, False, *into)
    check_bwd(rep, "[part into] ", out, g, x64, mean, invstd, w64, Lp, False, dw0.float().double(),
              db0.float().double(), into, sums=sums)
    out = m.bn_act_bwd(nhwc(_fresh(d["dy"]), 1, 1, M), mask, xs, mean, invstd, _fresh(d["w"]), _fresh(d["b"]), True,
                       True, None, None)
    dw_s, db_s = check_bwd(rep, "[stats] ", out, g, x64, mean, invstd, w64, Lb, True)
    rep.exact("dbeta part = stats", torch.equal(db_p, db_s))
    inv = invstd.double()
    e_both = inv * (sums[3] + bwd_sums(g, xc, Lb)[3]) + 2 * U * (inv * sums[1]).abs()
    rep.add("dgamma part vs stats", dw_p, dw_s.double(), e_both)
    rep.check()


# ---------------------------------------------------------------------------------------------
# 5. the pair: y = relu(BN(x) + BN_r(r))
# ---------------------------------------------------------------------------------------------
REPS, RMOM = f32(1e-3), f32(0.3)


@pytest.mark.parametrize("C,M,t,rt", [(16, 2403, 4, 64), (16, 2403, 64, 4), (24, 131, 7, 4), (8, 33000, 4, 7)],
                         ids=["x-merged", "r-merged", "small-nonhoisted", "M33000-both-merged"])
def test_bn_pair(cuda, C, M, t, rt):
    """bn_act_fwd_tiles_bnres and bn_act_bwd_pair: different tile_rows (one partial set merged, the
    other not, one merge buffer), different eps and momentum per side; the backward with one side
    accumulating into a prefilled gradient and the other returning it, and the reverse."""
    m = _m()
    dx_, dr_ = bn_inputs(M, C, 900 + M + t, cuda), ramp_inputs(M, C, 950 + M + rt, cuda)
    x64, r64 = dx_["x"].double(), dr_["x"].double()
    w64, b64, rw64, rb64 = dx_["w"].double(), dx_["b"].double(), dr_["w"].double(), dr_["b"].double()
    part, rpart = tile_partials(x64, t), tile_partials(r64, rt)
    G, rG = part.shape[0], rpart.shape[0]
    if M == 2403:
        assert (G > 512) != (rG > 512)
    if M == 33000:
        assert G > 512 and rG > 512 and stats_grid(M, C)[2] > 512
    _, _, e_mean, e_var, L = tiles_stats(part, t, M)
    _, _, re_mean, re_var, rL = tiles_stats(rpart, rt, M)
    Lb = chain_stats(M, C, True)
    assert max(L, rL, Lb) <= L_MAX
    rep = Report(f"pair C {C} M {M} tiles {t}/{rt} (L {L}/{rL}, bwd {Lb})")
    xs, rs = nhwc(_fresh(dx_["x"]), 1, 1, M), nhwc(_fresh(dr_["x"]), 1, 1, M)
    rm, rv, rrm, rrv = _fresh(dx_["rm"]), _fresh(dx_["rv"]), _fresh(dr_["rm"]), _fresh(dr_["rv"])
    y, mean, invstd, mask, rmean, rinvstd = m.bn_act_fwd_tiles_bnres(
        xs, _fresh(part), t, _fresh(dx_["w"]), _fresh(dx_["b"]), rm, rv, EPS, MOM,
        rs, _fresh(rpart), rt, _fresh(dr_["w"]), _fresh(dr_["b"]), rrm, rrv, REPS, RMOM, True)
    rref = bn_fwd_ref(r64, rw64, rb64, REPS, False)
    re_inv = invstd_bound(rref["var"], REPS, re_var)
    re_v = preact_bound(r64, rref["mean"], rref["invstd"], rw64, rb64, re_mean, re_inv)
    rref["e_mean"], rref["e_var"] = re_mean, re_var
    ref, _ = check_fwd(rep, "", x64, w64, b64, EPS, True, rows_of(y), mean, invstd, e_mean, e_var, rref["y"], re_v)
    rep.add("rmean", rmean, rref["mean"], re_mean)
    rep.add("rinvstd", rinvstd, rref["invstd"], re_inv)
    check_running(rep, "", rm, rv, dx_["rm"].double(), dx_["rv"].double(), ref, M, MOM)
    check_running(rep, "r ", rrm, rrv, dr_["rm"].double(), dr_["rv"].double(), rref, M, RMOM)
    ypos = rows_of(y) > 0
    rep.exact("mask", torch.equal(unpack_mask(mask, M, C), ypos))
    # backward
    g = dx_["dy"].double() * ypos
    for x_into in (True, False):
        tag = "[x into] " if x_into else "[r into] "
        dw0, db0 = (dx_["rm"] + 3.0), (dx_["rv"] - 2.0)
        a, b_ = _fresh(dw0), _fresh(db0)
        args = (a, b_, None, None) if x_into else (None, None, a, b_)
        dx, dr, dw, db, rdw, rdb = m.bn_act_bwd_pair(nhwc(_fresh(dx_["dy"]), 1, 1, M), mask, xs, mean, invstd,
                                                     _fresh(dx_["w"]), rs, rmean, rinvstd, _fresh(dr_["w"]), *args)
        for side, xx, mu, iv, ww, o_dx, o_dw, o_db, acc in (
                ("x ", x64, mean, invstd, w64, dx, dw, db, x_into),
                ("r ", r64, rmean, rinvstd, rw64, dr, rdw, rdb, not x_into)):
            mu64, iv64 = mu.double(), iv.double()
            xc = xx - mu64
            s1, s2, e_s1, e_s2 = bwd_sums(g, xc, Lb)
            dx_ref, dg_ref, db_ref = bn_bwd_ref(g, xx, mu64, iv64, ww)
            e_dx, e_dg, e_db = bwd_bound(s1, s2, e_s1, e_s2, g, xc, iv64, ww, M)
            rep.add(tag + side + "dx", rows_of(o_dx), dx_ref, out_bound(dx_ref, e_dx))
            if acc:
                assert o_dw.data_ptr() == a.data_ptr() and o_db.data_ptr() == b_.data_ptr()
                dg_ref, db_ref = dw0.double() + dg_ref, db0.double() + db_ref
                e_dg, e_db = e_dg + U * dg_ref.abs(), e_db + U * db_ref.abs()
            else:
                rep.exact(tag + side + "dbeta exact", torch.equal(o_db.double(), g.sum(0)))
            rep.add(tag + side + "dgamma", o_dw, dg_ref, e_dg)
            rep.add(tag + side + "dbeta", o_db, db_ref, e_db)
    rep.check()


# ---------------------------------------------------------------------------------------------
# 6. the stem: BatchNorm + ReLU + max-pool in one pass each way
# ---------------------------------------------------------------------------------------------
POOL_HW = [(1, 1), (2, 5), (9, 7), (16, 16), (15, 30)]
STEM_C = [8, 64, 2048]


def stem_inputs(N, C, H, W, seed, dev):
    """quantised x (window ties), mixed-sign γ, and β = −8 in every fifth channel so whole windows are
    ≤ 0 after the ReLU; integer dy for the pooled shape."""
    M = N * H * W
    x, w, b, _ = quantised_inputs(M, C, seed, "cpu")
    b = torch.where(torch.arange(C) % 5 == 4, torch.full_like(b, -8.0), b)
    g = torch.Generator().manual_seed(seed + 1)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randint(-4, 5, (N * OH * OW, C), generator=g).bfloat16()
    rm, rv = 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return tuple(v.to(dev) for v in (x, w, b, dy, rm, rv))


def check_stem(m, cuda, N, C, H, W, x, w, b, dy, rm0, rv0, rep, near_zero_beta=False):
    M, t = N * H * W, 7
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x64, w64, b64 = x.double(), w.double(), b.double()
    part = tile_partials(x64, t)
    _, _, e_mean, e_var, L = tiles_stats(part, t, M)
    Lb = chain_stats(N * OH * OW, C, True)
    assert max(L, Lb) <= L_MAX
    xs = nhwc(x, N, H, W)
    rm, rv = _fresh(rm0), _fresh(rv0)
    y, arg, xsel, mean, invstd = m.bn_relu_pool_fwd_tiles(xs, part, t, _fresh(w), _fresh(b), rm, rv, EPS, MOM)
    ref = bn_fwd_ref(x64, w64, b64, EPS, True)
    ref["e_mean"], ref["e_var"] = e_mean, e_var
    e_inv = invstd_bound(ref["var"], EPS, e_var)
    rep.add("mean", mean, ref["mean"], e_mean)
    rep.add("invstd", invstd, ref["invstd"], e_inv)
    check_running(rep, "", rm, rv, rm0.double(), rv0.double(), ref, M, MOM)
    # positions: inside the image, xsel = x[arg]
    arg4 = arg.view(N, OH, OW, C)
    assert int(arg4.max()) <= 8
    oh = torch.arange(OH, device=cuda)[None, :, None, None]
    ow = torch.arange(OW, device=cuda)[None, None, :, None]
    hh, ww = 2 * oh - 1 + arg4 // 3, 2 * ow - 1 + arg4 % 3
    rep.exact("arg inside", bool(((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)).all()))
    x4 = x.view(N, H, W, C)
    ysel = rows_of(y).view(N, OH, OW, C)
    xs4 = rows_of(xsel).view(N, OH, OW, C)
    rep.exact("xsel = x[arg]", same_bits(xs4, pool_gather(x4, arg4)))
    # y = bf16(relu(BN(xsel))), and no window element's activation lies above it
    act = ref["y"].view(N, H, W, C)
    e_v = preact_bound(x64, ref["mean"], ref["invstd"], w64, b64, e_mean, e_inv).view(N, H, W, C)
    bound = out_bound(act, e_v)
    rep.add("y", ysel, pool_gather(act, arg4), pool_gather(bound, arg4))
    below = torch.zeros((), dtype=F64, device=cuda)
    first_valid = torch.full_like(arg4, 255)
    earlier_equal = torch.zeros_like(arg4, dtype=torch.bool)
    for p, (a_p, b_p, x_p) in enumerate(zip(pool_windows(act, -math.inf), pool_windows(bound, 1.0),
                                            pool_windows(x4.double(), math.nan))):
        valid = ~torch.isnan(x_p)
        below = torch.maximum(below, torch.where(valid, (a_p - ysel.double()) / b_p, torch.zeros_like(a_p)).max())
        first_valid = torch.where(valid & (first_valid == 255), torch.full_like(arg4, p), first_valid)
        earlier_equal |= valid & (p < arg4) & (x_p == xs4.double())
    rep.rows.append(("window ≤ y", float(below)))
    rep.exact("first of equal inputs", not bool(earlier_equal.any()))
    rep.exact("all ≤ 0: first position", bool((arg4 == first_valid)[ysel == 0].all()))
    assert bool((ysel == 0).any()) and bool((ysel > 0).any())
    # backward: scatter dy to the chosen positions, ReLU mask, BatchNorm backward over the full M
    mu, inv = mean.double(), invstd.double()
    xsel64 = xs4.double().reshape(-1, C)
    if not near_zero_beta:
        dy = zero_near(dy, near_zero(xsel64, mu, inv, w64, b64))
    gp = dy.double() * (ysel.reshape(-1, C) > 0)  # pooled g: the forward's own y > 0
    gfull = pool_scatter(gp.view(N, OH, OW, C), arg4, H, W).reshape(M, C)
    xc = x64 - mu
    s1, s2, e_s1, e_s2 = bwd_sums(gp, xsel64 - mu, Lb)
    dx_ref, dg_ref, db_ref = bn_bwd_ref(gfull, x64, mu, inv, w64)
    e_dx, e_dg, e_db = bwd_bound(s1, s2, e_s1, e_s2, gfull, xc, inv, w64, M)
    dyp = nhwc(_fresh(dy), N, OH, OW)
    dx, dw, db = m.pool_bn_bwd(dyp, y, xsel, arg, xs, mean, invstd, _fresh(w), _fresh(b), None, None)
    rep.add("dx", rows_of(dx), dx_ref, out_bound(dx_ref, e_dx))
    rep.add("dgamma", dw, dg_ref, e_dg)
    rep.exact("dbeta exact", torch.equal(db.double(), db_ref))
    dw0, db0 = rm0 + 3.0, rv0 - 2.0
    a, b_ = _fresh(dw0), _fresh(db0)
    dx2, dw2, db2 = m.pool_bn_bwd(dyp, y, xsel, arg, xs, mean, invstd, _fresh(w), _fresh(b), a, b_)
    assert dw2 is None and db2 is None
    rep.exact("dx again", same_bits(dx2, dx))
    rep.add("dgamma into", a, dw0.double() + dg_ref, e_dg + U * (dw0.double() + dg_ref).abs())
    rep.add("dbeta into", b_, db0.double() + db_ref, U * (db0.double() + db_ref).abs())
    return L, Lb


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("HW", POOL_HW, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", STEM_C)
def test_stem_bn_relu_pool(cuda, C, HW, N):
    H, W = HW
    m = _m()
    x, w, b, dy, rm, rv = stem_inputs(N, C, H, W, stem_seed(N, C, H, W), cuda)
    rep = Report(f"stem N {N} C {C} {H}x{W}")
    L, Lb = check_stem(m, cuda, N, C, H, W, x, w, b, dy, rm, rv, rep)
    rep.what += f" (L {L}, bwd {Lb})"
    rep.check()


def test_stem_recomputed_mask(cuda):
    """pool_bn_bwd's apply pass recomputes the ReLU mask at full resolution while its statistics read
    y: with a frequent input value within a few ulps of zero, dy non-zero only where the window's
    maximum is positive must still give the scatter reference."""
    m = _m()
    N, C, H, W = 2, 64, 15, 30
    x, w, b, dy, rm, rv = stem_inputs(N, C, H, W, 99, cuda)
    M = N * H * W
    part = tile_partials(x.double(), 7)
    _, _, _, mean, invstd = m.bn_relu_pool_fwd_tiles(nhwc(x, N, H, W), part, 7, w, b, None, None, EPS, MOM)
    # x* = the second largest grid value for γ > 0 (the smallest but one for γ < 0): often a window's maximum
    xstar = torch.where(w > 0, torch.full_like(w, 2.5), torch.full_like(w, -2.5)).bfloat16()
    b0 = beta_for_zero(xstar, mean, invstd, w)
    y = m.bn_relu_pool_fwd_tiles(nhwc(x, N, H, W), part, 7, w, b0, None, None, EPS, MOM)[0]
    dy = torch.where(rows_of(y) > 0, dy, torch.zeros_like(dy))
    rep = Report("stem, x* at the ReLU's zero")
    check_stem(m, cuda, N, C, H, W, x, w, b0, dy, rm, rv, rep, near_zero_beta=True)
    rep.check()


def test_stem_rejects_c24(cuda):
    m = _m()
    N, C, H, W = 1, 24, 4, 4
    x, w, b, dy, rm, rv = stem_inputs(N, C, H, W, 1, cuda)
    part = tile_partials(x.double(), 7)
    with pytest.raises(RuntimeError):
        m.bn_relu_pool_fwd_tiles(nhwc(x, N, H, W), part, 7, w, b, None, None, EPS, MOM)
    z = nhwc(torch.zeros(N * 2 * 2, C, device=cuda, dtype=BF16), N, 2, 2)
    arg = torch.zeros(N * 2 * 2 * C, device=cuda, dtype=torch.uint8)
    mean, invstd = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    with pytest.raises(RuntimeError):
        m.pool_bn_bwd(z, z.clone(), z.clone(), arg, nhwc(x, N, H, W), mean, invstd, w, b, None, None)


# ---------------------------------------------------------------------------------------------
# 7. pooling alone, exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", POOL_HW + [(3, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [8, 40, 64])
def test_maxpool3s2_exact(cuda, C, HW):
    """tie-heavy integer inputs: y, arg and dx bit for bit, a pixel that is the maximum of four windows
    included; (3, 70) at C = 64 is a row wider than 256 lanes (OW·C/8 = 280)."""
    m = _m()
    H, W = HW
    N = 2
    g = torch.Generator().manual_seed(C * 100 + H * 7 + W)
    x = torch.randint(-2, 3, (N, H, W, C), generator=g).float()
    four = H >= 4 and W >= 4
    if four:
        x[:, 1, 1, :] = 9.0  # the maximum of windows (0,0), (0,1), (1,0), (1,1)
    x = x.bfloat16().to(cuda)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if HW == (3, 70) and C == 64:
        assert OW * C // 8 > 256
    dy = torch.randint(-4, 5, (N, OH, OW, C), generator=g).bfloat16().to(cuda)
    y, arg = m.maxpool3s2_fwd(x.permute(0, 3, 1, 2))
    y_ref, arg_ref = pool_fwd_ref(x)
    assert same_bits(y.permute(0, 2, 3, 1).contiguous(), y_ref)
    assert torch.equal(arg.permute(0, 2, 3, 1), arg_ref)
    dx = m.maxpool3s2_bwd(dy.permute(0, 3, 1, 2), arg, H, W)
    dx_ref = pool_scatter(dy.double(), arg_ref, H, W)
    assert same_bits(dx.permute(0, 2, 3, 1).contiguous(), dx_ref.bfloat16())
    if four:
        want = dy[:, :2, :2].double().sum((1, 2))
        assert torch.equal(dx.permute(0, 2, 3, 1)[:, 1, 1].double(), want)


@pytest.mark.parametrize("shape", [(4, 64, 5, 5), (3, 8, 1, 1)], ids=["4x64x5x5", "3x8x1x1"])
def test_gap_bwd_exact(cuda, shape):
    """dx = bf16(fp32(dy)·fp32(1/HW)) at every pixel, bit for bit."""
    m = _m()
    N, C, H, W = shape
    dy = torch.randn(N, C, generator=torch.Generator().manual_seed(N)).bfloat16().to(cuda)
    dx = m.gap_bwd(dy, H, W)
    assert dx.shape == (N, C, H, W) and dx.is_contiguous(memory_format=torch.channels_last)
    inv = float(np.float32(1.0) / np.float32(H * W))
    want = (dy.double() * inv).float().bfloat16()  # an 8-bit by 24-bit product is exact in float64
    assert same_bits(dx, want[:, :, None, None].expand(N, C, H, W))
