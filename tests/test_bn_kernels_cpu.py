"""CPU self-checks of the float64 references, input builders and bounds that test_bn_kernels_gpu.py
holds the BatchNorm and pooling kernels to: every reference against float64 autograd, the partials
builder against var(x) through the documented merge, the near-zero share of the chosen seeds."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_bn_kernels_gpu import (ALL_MODES, EPS, LARGE, MOM, POOL_HW, STATS_C, STATS_M, STEM_C, U, beta_for_zero,
                                 bn_bwd_ref, bn_fwd_ref, bn_inputs, bn_stats_ref, bwd_partials, chain_rows,
                                 chain_stats, chain_tiles, fwd_stats_bound, group_sizes, invstd_bound, merge_level,
                                 near_zero, pool_fwd_ref, pool_gather, pool_scatter, quantised_inputs, ramp_inputs,
                                 running_ref, stats_grid, stats_seed, stem_inputs, stem_seed, tile_counts,
                                 tile_partials, tiles_M, tiles_stats, unpack_mask)

F64 = torch.float64
TOL = 1e-12


def _close(got, want, what):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= TOL * max(scale, 1e-300), f"{what}: {err:.3e} against a scale of {scale:.3e}"


@pytest.mark.parametrize("relu,use_res", ALL_MODES)
def test_bn_references_match_autograd_fp64(relu, use_res):
    """bn_fwd_ref, running_ref and bn_bwd_ref against torch.nn.functional.batch_norm (+ residual, ReLU)
    and its autograd in float64, γ < 0 and γ = 0 channels included; no pre-activation ties at zero."""
    M, C = 200, 24
    d = bn_inputs(M, C, 1)
    g = torch.Generator().manual_seed(2)
    x = d["x"].double() + 1e-3 * torch.randn(M, C, generator=g, dtype=F64)  # the constant channel gets a spread
    w, b, res = d["w"].double(), d["b"].double(), d["res"].double()
    dy = torch.randn(M, C, generator=g, dtype=F64)
    xa, wa, ba, ra = (t.clone().requires_grad_() for t in (x, w, b, res))
    rm, rv = d["rm"].double(), d["rv"].double()
    rm_t, rv_t = rm.clone(), rv.clone()
    out = F.batch_norm(xa.t()[None], rm_t, rv_t, wa, ba, True, MOM, EPS)[0].t()  # [1, C, M] layout
    if use_res:
        out = out + ra
    if relu:
        out = F.relu(out)
    out.backward(dy)
    ref = bn_fwd_ref(x, w, b, EPS, relu, res if use_res else None)
    _close(ref["y"], out.detach(), "y")
    rm_r, rv_r = running_ref(rm, rv, ref["mean"], ref["var"], M, MOM)
    _close(rm_r, rm_t, "running mean")
    _close(rv_r, rv_t, "running var (unbiased)")
    gm = dy * (ref["pre"] > 0) if relu else dy
    dx, dg, db = bn_bwd_ref(gm, x, ref["mean"], ref["invstd"], w)
    _close(dx, xa.grad, "dx")
    _close(dg, wa.grad, "dgamma")
    _close(db, ba.grad, "dbeta")
    if use_res:
        _close(gm, ra.grad, "dres")


def test_running_variance_factor_is_one_at_m1():
    """documented: unbiased factor M / (M − 1), and 1 at M = 1 (where var = 0 anyway)."""
    rm, rv = torch.tensor([0.5], dtype=F64), torch.tensor([2.0], dtype=F64)
    mean, var = torch.tensor([3.0], dtype=F64), torch.tensor([0.25], dtype=F64)
    a, b = running_ref(rm, rv, mean, var, 1, 0.1)
    assert float(a) == 0.9 * 0.5 + 0.1 * 3.0 and float(b) == 0.9 * 2.0 + 0.1 * 0.25
    _, b4 = running_ref(rm, rv, mean, var, 4, 0.1)
    assert abs(float(b4) - (0.9 * 2.0 + 0.1 * 0.25 * 4 / 3)) < 1e-15


@pytest.mark.parametrize("t", [4, 7])
@pytest.mark.parametrize("G", [1, 5, 512, 513, 600, 1100])
def test_partials_reproduce_var(G, t):
    """the builder's rows through the documented merge, and through 256-row chunks first, give var(x);
    the fp32-rounded rows stay within the bound tiles_stats derives for them."""
    M, C = tiles_M(G, t), 16
    assert (M + t - 1) // t == G and M % t != 0
    x = ramp_inputs(M, C, 31 * G + t)["x"].double()
    mean, var = bn_stats_ref(x)
    p = tile_partials(x, t, F64)
    n = tile_counts(M, t, "cpu")
    assert float(n.sum()) == M and float(n[-1]) < t
    S, Q, _, _ = merge_level(p[:, 0], p[:, 1], n)
    _close(S / M, mean, "mean, one level")
    _close(Q / M, var, "var, one level")
    chunks = [merge_level(p[i:i + 256, 0], p[i:i + 256, 1], n[i:i + 256]) for i in range(0, G, 256)]
    cn = torch.stack([n[i:i + 256].sum() for i in range(0, G, 256)])
    S2, Q2, _, _ = merge_level(torch.stack([c[0] for c in chunks]), torch.stack([c[1] for c in chunks]), cn)
    _close(S2 / M, mean, "mean, two levels")
    _close(Q2 / M, var, "var, two levels")
    p32 = tile_partials(x, t)
    assert p32.dtype == torch.float32 and torch.equal(p32, p.float())
    m_t, v_t, e_mean, e_var, L = tiles_stats(p32, t, M)
    assert L == (chain_tiles(G) if G <= 512 else 8 + chain_tiles((G + 255) // 256)) and L <= 19
    assert bool(((m_t - mean).abs() <= e_mean).all()) and bool(((v_t - var).abs() <= e_var).all())
    if M > 1:
        assert float((e_var / var).max()) < 1e-4  # the bound has teeth: a dropped between-tile term is O(1)


def test_bwd_partials_sum_to_the_totals():
    G = 513
    sizes = group_sizes(G)
    M = int(sizes.sum())
    assert len(set(sizes.tolist())) == 5
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(M, 8, generator=g, dtype=F64), torch.randn(M, 8, generator=g, dtype=F64)
    p = bwd_partials(a, b, sizes)
    assert p.shape == (G, 2, 8) and p.dtype == torch.float32
    assert float((p[:, 0].double().sum(0) - a.sum(0)).abs().max()) < 1e-4
    assert float((p[:, 1].double().sum(0) - (a * b).sum(0)).abs().max()) < 1e-4
    assert torch.equal(p[0, 0].double(), a[0].float().double())  # group 0 is row 0, group 1 rows 1 and 2
    assert float((p[1, 0].double() - a[1:3].sum(0)).abs().max()) < 1e-6


@pytest.mark.parametrize("HW", POOL_HW + [(3, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool_references_match_max_pool2d(HW):
    H, W = HW
    N, C = 2, 8
    g = torch.Generator().manual_seed(H * 100 + W)
    a = torch.randn(N, H, W, C, generator=g, dtype=F64)  # no ties
    dy = torch.randn(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, generator=g, dtype=F64)
    aa = a.clone().requires_grad_()
    y = F.max_pool2d(aa.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    y.backward(dy)
    best, arg = pool_fwd_ref(a)
    assert torch.equal(best, y.detach())
    assert torch.equal(pool_gather(a, arg), best)
    _close(pool_scatter(dy, arg, H, W), aa.grad, "dx")  # up to the order of ≤ 4 additions


def test_pool_reference_ties_and_edges():
    a = torch.zeros(1, 4, 4, 1, dtype=F64)
    best, arg = pool_fwd_ref(a)
    # all equal: the first valid position in (kh, kw) order: (1,1) at the corner, (1,0) / (0,1) on an edge, (0,0) inside
    assert arg[0, :, :, 0].tolist() == [[4, 3], [1, 0]]
    a[0, 1, 1, 0] = 9.0
    best, arg = pool_fwd_ref(a)
    assert arg[0, :, :, 0].tolist() == [[8, 6], [2, 0]] and bool((best == 9.0).all())  # the maximum of four windows
    dy = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=F64).view(1, 2, 2, 1)
    dx = pool_scatter(dy, arg, 4, 4)
    assert float(dx[0, 1, 1, 0]) == 10.0 and float(dx.sum()) == 10.0
    assert math.isnan(float(pool_gather(a, torch.zeros_like(arg))[0, 0, 0, 0]))  # position 0 of window (0,0) is padding


def test_stem_reference_matches_autograd_fp64():
    """BN → ReLU → max-pool, and scatter → ReLU mask → BN backward over the full-resolution M."""
    N, C, H, W = 2, 8, 9, 7
    M = N * H * W
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, C, generator=g, dtype=F64)
    w = torch.randn(C, generator=g, dtype=F64)
    b = 0.3 * torch.randn(C, generator=g, dtype=F64)
    dy = torch.randn(N, 5, 4, C, generator=g, dtype=F64)
    xa, wa, ba = (t.clone().requires_grad_() for t in (x, w, b))
    z = F.relu(F.batch_norm(xa.view(N, H, W, C).permute(0, 3, 1, 2), None, None, wa, ba, True, MOM, EPS))
    y = F.max_pool2d(z, 3, 2, 1).permute(0, 2, 3, 1)
    y.backward(dy)
    ref = bn_fwd_ref(x, w, b, EPS, True)
    best, arg = pool_fwd_ref(ref["y"].view(N, H, W, C))
    _close(best, y.detach(), "pooled y")
    xsel = pool_gather(x.view(N, H, W, C), arg)
    _close(((xsel - ref["mean"]) * ref["invstd"] * w + b).clamp_min(0), best, "relu(BN(xsel))")
    gp = dy * (best > 0)
    gfull = pool_scatter(gp, arg, H, W).reshape(M, C)
    dx, dg, db = bn_bwd_ref(gfull, x, ref["mean"], ref["invstd"], w)
    _close(dx, xa.grad, "dx")
    _close(dg, wa.grad, "dgamma")
    _close(db, ba.grad, "dbeta")
    # the backward kernel's statistics run over the pooled tensors: the same sums
    _close(gp.reshape(-1, C).sum(0), gfull.sum(0), "Σg pooled")
    _close((gp * (xsel - ref["mean"])).reshape(-1, C).sum(0), (gfull * (x - ref["mean"])).sum(0), "Σg·xc pooled")


def test_chain_lengths():
    """the launch geometry the bounds count: L ≤ 29 for every shape of the GPU file (28 without the
    backward's bn_sum_rows level)."""
    assert stats_grid(33000, 8)[2] == 516 and stats_grid(135200, 64)[1:] == (1, 2048, 67)
    assert chain_stats(135200, 64, False) == 3 + 5 + 8 + 9 and chain_stats(135200, 64, True) == 3 + 5 + 8 + 1 + 9
    assert chain_stats(360000, 24, False) == 6 + 5 + 8 + 9 == 28 and chain_stats(360000, 24, True) == 29
    assert chain_stats(200, 2048, True) == 7 + 3 + 1 + 9
    assert chain_rows(512, True) == 2 + 9 and chain_rows(513, True) == 8 + 1 + 9 and chain_rows(513, False) == 3 + 9
    assert chain_tiles(512) == 11 and chain_tiles(1100) == 14
    shapes = [(M, C) for C in STATS_C for M in STATS_M] + [(s[0] * s[2] * s[3], s[1]) for s, _ in LARGE]
    assert max(chain_stats(M, C, mg) for M, C in shapes for mg in (False, True)) == 29


def _f32_mean_inv(x, eps):
    mean, var = bn_stats_ref(x)
    return mean.float().double(), ((var + eps) ** -0.5).float().double()


def test_near_zero_share_of_the_chosen_seeds():
    """under 0.1 % of the pre-activations lie within the fp32 bound of zero, for every input set a
    mask-recomputing backward is given (mean and invstd: the float64 ones rounded to fp32)."""
    worst = 0.0
    cases = [(M, C) for C in STATS_C for M in STATS_M] + [(2 * 260 * 260, 64)]
    for M, C in cases:
        d = bn_inputs(M, C, stats_seed(C, M))
        x, w, b = d["x"].double(), d["w"].double(), d["b"].double()
        mean, inv = _f32_mean_inv(x, EPS)
        share = float(near_zero(x, mean, inv, w, b).double().mean())
        worst = max(worst, share)
        assert share < 1e-3, (M, C, share)
    print(f"worst near-zero share, stats pass: {worst:.2e}")


@pytest.mark.parametrize("C", STEM_C)
def test_stem_inputs_have_ties_dead_windows_and_few_near_zero(C):
    for H, W in POOL_HW:
        for N in (1, 3):
            M = N * H * W
            x, w, b, dy, rm, rv = stem_inputs(N, C, H, W, stem_seed(N, C, H, W), "cpu")
            x64, w64, b64 = x.double(), w.double(), b.double()
            assert bool((w > 0).any()) and bool((w < 0).any())
            ref = bn_fwd_ref(x64, w64, b64, EPS, True)
            act = ref["y"].bfloat16().double().view(N, H, W, C)
            best, arg = pool_fwd_ref(act)
            assert bool((best == 0).any()) and bool((best > 0).any()), (N, C, H, W)
            if H * W >= 35:
                wins = torch.stack([torch.nan_to_num(v, nan=-1.0) for v in
                                    [pool_gather(act, torch.full_like(arg, p)) for p in range(9)]])
                assert bool(((wins == best).sum(0) > 1)[best > 0].any()), "no window holds a tie"
            mean, inv = _f32_mean_inv(x64, EPS)
            xsel = pool_gather(x64.view(N, H, W, C), arg).reshape(-1, C)
            assert float(near_zero(xsel, mean, inv, w64, b64).double().mean()) < 1e-3


def test_shifted_variance_claim():
    """x = 64 + 0.5k, k ∈ [−4, 4], M = 4000: with fully sequential fp32 sums the row-0-shifted invstd is
    within 1e-8 relative of float64 and far inside the bound at L = 30; the unshifted E[x²] − E[x]² is
    off by more than 1e-3, four orders of magnitude above the bound."""
    rng = np.random.RandomState(0)
    x = (64 + 0.5 * rng.randint(-4, 5, 4000)).astype(np.float32)
    var64 = float(np.var(x.astype(np.float64)))
    inv64 = (var64 + EPS) ** -0.5
    f = np.float32
    d = x - x[0]
    s, q, s0, q0 = f(0), f(0), f(0), f(0)
    for i in range(x.size):
        s, q = f(s + d[i]), f(q + f(d[i] * d[i]))
        s0, q0 = f(s0 + x[i]), f(q0 + f(x[i] * x[i]))
    Minv = f(1) / f(x.size)
    md = f(s * Minv)
    var = f(f(q * Minv) - f(md * md))
    m0 = f(s0 * Minv)
    var0 = max(f(f(q0 * Minv) - f(m0 * m0)), f(0))
    inv, inv0 = float(var + f(EPS)) ** -0.5, float(var0 + f(EPS)) ** -0.5
    xt = torch.tensor(x, dtype=F64)[:, None]
    _, e_var = fwd_stats_bound(xt, 30)
    bound = float(invstd_bound(torch.tensor([var64], dtype=F64), EPS, e_var)) / inv64
    print(f"shifted {abs(inv - inv64) / inv64:.2e}  unshifted {abs(inv0 - inv64) / inv64:.2e}  bound {bound:.2e}")
    assert abs(inv - inv64) / inv64 < 1e-6 and abs(inv - inv64) / inv64 < bound
    assert abs(inv0 - inv64) / inv64 > 1e-3 > 100 * bound


def test_beta_for_zero_is_within_a_few_ulps():
    x, w, b, _ = quantised_inputs(500, 24, 29, "cpu")
    mean, inv = (t.float() for t in _f32_mean_inv(x.double(), EPS))
    xstar = x[1]
    b0 = beta_for_zero(xstar, mean, inv, w)
    sc = w.double() * inv.double()
    pre = (xstar.double() - mean.double()) * sc + b0.double()
    scale = (xstar.double() * sc).abs() + (mean.double() * sc).abs()
    assert bool((pre.abs() <= 8 * U * scale + 1e-30).all())
    assert len({round(float(v), 12) for v in (pre / (U * scale))}) > 3  # not all on one side, not all alike


def test_unpack_mask_bit_order():
    mask = torch.tensor([0b00000101, 0b10000000], dtype=torch.uint8)
    assert unpack_mask(mask, 2, 8).tolist() == [[True, False, True] + [False] * 5, [False] * 7 + [True]]
    assert unpack_mask(mask, 1, 16).shape == (1, 16)
