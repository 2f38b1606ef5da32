"""CPU self-checks of what test_resnet_nodes_gpu.py holds the ResNet autograd nodes to: the route helpers,
hooks and counters; the route predicates of ops/resnet.py on the table's shapes (the extension's
gemm_nt_supported repeated as arithmetic); the grid cases' exactness preconditions, the mask packing and
the shares in which the rounding contracts differ; a faithful fp32 emulation of each contract (it passes,
and the float64 reference alone stays inside every band); and the checkers on perturbed results — one
dropped pixel, a mask shifted by one byte, applied twice or not at all, a compact add at transposed
pixels, an arena overwrite, the partials of the wrong tensor, dx and dres swapped — each must fail."""
import pytest
import torch
import torch.nn.functional as F

import test_bn_kernels_gpu as bk
import test_conv_exact_gpu as cx
import test_resnet_nodes_gpu as rn
from test_bn_kernels_gpu import EPS, L_MAX, U, Report, bn_bwd_ref, chain_rows, chain_stats, check_bwd, out_bound, tiles_stats, unpack_mask
from test_conv_exact_gpu import KRSC, NHWC, check_bits, exact_f32, first_mismatch, nhwc, rne_bf16, stride2_add_ref
from test_resnet_nodes_gpu import (BIG, BLOCK_CASES, BLOCKS, CONV_NODE, DS_CASES, FWD_ROUTES, IDENT, LT, STEM_ROUTES,
                                   check_fwd_given, conv_bound, conv_node_expect, ds_case, ds_expect, dx_expect,
                                   expected_links, ident_case, keep_of, nt4, pack_mask, relu_res_expect, rne2, zero_fill)

BF16 = torch.bfloat16
F64 = torch.float64
DIFFER_MIN = 0.05   # share of elements in which two contracts must differ for a test to tell them apart


def record(line):
    print(f"[resnet-nodes-cpu] {line}")


def share(mask):
    return float(mask.double().mean())


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


class FakeExt:
    """gemm_nt_supported as arithmetic (gemm_nt.hip gemm_nt_ok at lda = ldb = K, ldc = N): M % 256 = 0,
    K % 64 = 0, K >= 64, and N % 256 = 0 or, on the 4-wave mainloop, N % 256 = 128."""

    @staticmethod
    def gemm_nt_supported(M, N, K):
        return M > 0 and M % 256 == 0 and K >= 64 and K % 64 == 0 and (N % 256 == 0 or (N % 256 == 128 and nt4(K)))


# ---------------------------------------------------------------------------------------------
# routes, hooks, counters
# ---------------------------------------------------------------------------------------------
def test_route_helpers_hooks_and_counters():
    from paddle_operator_amd.ops import resnet as R
    x = torch.ones(3, requires_grad=True)
    y = (x * 2).exp().sum()
    order = [type(f).__name__ for f in rn.graph_nodes(y)]
    assert order[:3] == ["SumBackward0", "ExpBackward0", "MulBackward0"] and "AccumulateGrad" in order
    assert rn.tap(y) == []                                   # no project node in a framework graph
    rejects(rn.assert_route, y, ["_ConvFn"])                 # a route that was not taken fails
    names = ("_BN_LINK", "_RES_MASK", "_DS_COMPACT", "_DS_FUSED", "_GEMM_BN_STATS", "_HIP_CONV", "_HIP_STEM", "_STEM_POOL",
             "_BN_FUSED")
    before = tuple(getattr(R, k)[0] for k in names)
    with pytest.raises(RuntimeError):
        with rn.hooks(**{k: False for k in names}):
            assert not any(getattr(R, k)[0] for k in names)
            raise RuntimeError("inside")
    assert tuple(getattr(R, k)[0] for k in names) == before
    with rn.links() as lk:
        assert lk.used == (0, 0, 0)
        R._ResMaskLink().take(None)                          # nothing given: no mask, no count
        assert lk.used == (0, 0, 0)
        link = R._CompactGradLink()
        link.give(torch.ones(1))
        link.take()
        assert lk.used == (0, 0, 1)
        t = torch.ones(2)
        rl = R._ResMaskLink()
        rl.give(t, torch.zeros(1, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="residual mask hand-off"):
            rl.take(t + 0)                                   # another tensor: raised, never masked
        assert lk.used == (0, 0, 1)
    # every table names hooks and node classes that exist
    have = set(dir(R))
    for table in (FWD_ROUTES.values(), STEM_ROUTES.values()):
        for entry in table:
            hk = next(e for e in entry if isinstance(e, dict))
            assert all(h in have for h in hk)
            assert all(n in have for lst in entry if isinstance(lst, list) for n in lst)
    assert all(h in have for _, hk in BLOCK_CASES for h in hk) and all(k in BLOCKS for k, _ in BLOCK_CASES)
    for n in rn.WATCH:
        assert n[:-len("Backward")] in have
    assert len({rn.case_id(c) for c in BLOCK_CASES}) == len(BLOCK_CASES)


def test_route_predicates_on_the_table_shapes():
    """_gemm_fwd_1x1, _gemm_dgrad_1x1, _gemm_wgrad_1x1 and the compact GEMM's gate at T256, T147 and the two
    stride-2 shapes; every CONV_NODE entry lists the calls the predicates select."""
    from paddle_operator_amd.ops import resnet as R
    m = FakeExt()
    T256, T147 = 4 * 8 * 8, 3 * 7 * 7
    assert R._gemm_fwd_1x1(m, T256, 256, 512) and R._gemm_fwd_1x1(m, T256, 64, 256)      # 4-wave, 8-wave
    assert not R._gemm_fwd_1x1(m, T256, 256, 64) and not R._gemm_fwd_1x1(m, T256, 256, 128)   # Kout <= 128
    assert not R._gemm_fwd_1x1(m, T147, 256, 512)
    assert nt4(256) and nt4(512) and not nt4(64) and not nt4(128) and not nt4(320)
    assert R._gemm_dgrad_1x1(m, T256, 256, 64) and R._gemm_dgrad_1x1(m, T256, 256, 512) and R._gemm_dgrad_1x1(m, T256, 2048, 512)
    assert not R._gemm_dgrad_1x1(m, T256, 64, 256) and not R._gemm_dgrad_1x1(m, T256, 128, 512)   # Cin <= 128
    assert not R._gemm_dgrad_1x1(m, T147, 256, 512)
    assert not R._gemm_dgrad_1x1(m, 3 * 14 * 14, 256, 256)                  # 588 tokens: conv1 of the 14 x 14 block
    assert R._gemm_wgrad_1x1(2048, 512) and not R._gemm_wgrad_1x1(256, 512) and not R._gemm_wgrad_1x1(1024, 256)
    assert T256 % 64 == 0 and T147 % 64 != 0                                # gemm_dw's 64-token k-tile
    assert m.gemm_nt_supported(2 * 8 * 16, 256, 512) and not m.gemm_nt_supported(3 * 7 * 7, 256, 512)   # the compact GEMM
    for name, (shape, alias, arena, route, want) in CONV_NODE.items():
        N, C, H, W, K, R_, st = shape
        T, one = N * H * W, R_ == 1 and st == 1
        assert ("gemm_nt_stats" in want) == (one and R._gemm_fwd_1x1(m, T, C, K)), name
        assert ("conv_fwd" in want) != ("gemm_nt_stats" in want), name
        assert (route == "gemm") == (one and R._gemm_dgrad_1x1(m, T, C, K)), name
        assert (route == "gemm") == ("gemm_nt" in want or "gemm_nt_add" in want) == ("transpose" in want), name
        assert (route == "dgrad") == ("conv_dgrad" in want) == ("conv_weight_t" in want), name
        assert ("gemm_nt_add" in want) == (route == "gemm" and alias != "none"), name
        assert ("gemm_dw" in want) == (one and R._gemm_wgrad_1x1(C, K)), name
        assert ("conv_wgrad" in want) == (not ("gemm_dw" in want and T % 64 == 0)), name
    for name, (dims, hook, contract, route) in DS_CASES.items():
        N, C, H, W, K1, Kd = dims
        To = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        assert (contract == "compact") == (hook and m.gemm_nt_supported(To, C, Kd)), name
        assert (route == "gemm") == R._gemm_dgrad_1x1(m, N * H * W, C, K1) and nt4(K1), name
    for key, (N, C, H, W, K) in IDENT.items():
        assert key.startswith("gemm") == R._gemm_dgrad_1x1(m, N * H * W, C, K)
    want = {("ident-T256", ()): (2, 1, 0), ("ident-T147", ()): (2, 1, 0), ("ident-wide-T256", ()): (1, 1, 0),
            ("ident-T256", ("_BN_LINK",)): (0, 1, 0), ("ident-T256", ("_RES_MASK",)): (2, 0, 0),
            ("ds2-16x32", ()): (2, 0, 1), ("ds2-16x32", ("_DS_FUSED",)): (2, 1, 1),
            ("ds2-16x32", ("_DS_FUSED", "_RES_MASK")): (2, 0, 1), ("ds2-16x32", ("_DS_COMPACT",)): (2, 0, 0),
            ("ds2-14x14", ()): (2, 0, 0), ("ds2-14x14", ("_DS_FUSED",)): (2, 1, 0), ("ds1-T256", ()): (2, 0, 0)}
    for (kind, off), links in want.items():
        assert expected_links(kind, {k: False for k in off}, m) == links, (kind, off)
    # every link counter moves in some block case, and stays in another
    moved = [expected_links(k, hk, m) for k, hk in BLOCK_CASES]
    for i in range(3):
        assert any(u[i] for u in moved) and not all(u[i] for u in moved)


# ---------------------------------------------------------------------------------------------
# (a) the grid cases
# ---------------------------------------------------------------------------------------------
def test_mask_packing_is_unpack_masks_inverse():
    N, C, H, W = 2, 16, 3, 5
    keep = keep_of((N, C, H, W), 3)
    bits = pack_mask(keep)
    assert bits.dtype == torch.uint8 and bits.numel() == N * C * H * W // 8
    assert torch.equal(unpack_mask(bits, N * H * W, C), bk.rows_of(keep))
    from paddle_operator_amd.ops import _apply_bitmask
    t = torch.arange(N * C * H * W, dtype=torch.float32).view(N, H, W, C).permute(0, 3, 1, 2) + 1.0
    assert torch.equal(_apply_bitmask(t, bits), t * keep)
    assert 0.4 < share(keep) < 0.6


@pytest.mark.parametrize("name", list(CONV_NODE))
def test_conv_node_cases_exact_and_telling(name):
    """Every expected tensor is bf16- / fp32-exact (the builders assert the 2^24 bounds); a masked case's
    expectation differs from the unmasked and from the twice-shifted one in a useful share of elements."""
    shape, alias, arena, route, want = CONV_NODE[name]
    e = conv_node_expect(name)
    c = e["c"]
    N, C, H, W, K, R, st = shape
    assert e["y"].dtype == BF16 and e["dx"].dtype == BF16
    exact_f32(c["base"] + e["dw"])
    if alias == "mask":
        plain = dx_expect(c["dx"], c["add"], route, K)
        d = share(plain != e["dx"])
        record(f"{name}: masked and unmasked dX differ in {d:.1%}")
        assert d >= DIFFER_MIN
    if alias != "none" and route == "gemm":
        # |P| <= Kout DY_MAX W_MAX: on the 8-wave ring the product is bf16-exact here, the two contracts coincide
        two = rne2(c["dx"], c["add"] * e["keep"] if alias == "mask" else c["add"])
        if not nt4(K):
            assert K * cx.DY_MAX * cx.W_MAX <= 256 and torch.equal(two, e["dx"])
    if "gemm_dw" in want and "conv_wgrad" not in want:
        d = share(e["dw"] != c["dw"])
        record(f"{name}: RNE_bf16(dW) differs from the exact dW in {d:.1%}")
        assert d >= DIFFER_MIN


def test_identity_cases():
    for key in IDENT:
        k = ident_case(key)
        c = k["c"]
        N, C, H, W, K = IDENT[key]
        assert k["yo"].dtype == BF16 and float(k["dyo"].abs().max()) <= cx.ADD_MAX
        assert cx.exact_bound(K, cx.DY_MAX, cx.W_MAX, cx.ADD_MAX) < cx.LIM
        assert float(k["g"].abs().sum((0, 2, 3)).max()) < cx.LIM         # dbeta sums exactly
        route = "gemm" if key.startswith("gemm") else "dgrad"
        masked, plain = dx_expect(c["dx"], k["g"], route, K), dx_expect(c["dx"], k["dyo"], route, K)
        assert share(masked != plain) >= DIFFER_MIN
        # gamma = 0 in fp32, as the kernel forms it: x sc + sh with sc = 0, sh = beta - mean 0
        x3 = torch.randn(N, C, H, W)
        mean = x3.mean((0, 2, 3), keepdim=True)
        sc = torch.zeros(1, C, 1, 1)
        v = x3 * sc + (k["beta"].float().view(1, C, 1, 1) - mean * sc) + c["x"].float()
        assert torch.equal(v.clamp_min(0).to(BF16), k["yo"]) and torch.equal(v > 0, k["keep"])


def test_compact_and_zero_filled_contracts_differ():
    """On the chosen magnitudes the compact contract (two roundings at (2a, 2b)) and the zero-filled one (one)
    differ in at least 5 % of the stride-2 pixels; on the 8-wave ring they coincide; the fp32 emulations of
    both give the expected bits."""
    dims = DS_CASES["compact-16x32"][0]
    N, C, H, W, K1, Kd = dims
    k = ds_case(*dims)
    comp, one = ds_expect(k["p1"], k["pds"], True), ds_expect(k["p1"], k["pds"], False, "gemm", K1)
    d = share(comp[:, :, ::2, ::2] != one[:, :, ::2, ::2])
    record(f"compact and zero-filled dX differ in {d:.1%} of the stride-2 pixels")
    assert d >= DIFFER_MIN
    off = torch.ones(H, W, dtype=torch.bool)
    off[::2, ::2] = False
    assert torch.equal(comp[:, :, off], one[:, :, off])
    assert torch.equal(ds_expect(k["p1"], k["pds"], False, "gemm", 64), comp)       # 8-wave: the same two roundings
    assert torch.equal(ds_expect(k["p1"], k["pds"], False, "dgrad", K1), one)
    # fp32 emulation: sums of integers below 2^24 in fp32, in another order, then the contract's roundings
    p1 = (k["dy1"].float().flip(1).permute(0, 2, 3, 1) @ k["w1"].float().flip(0).view(K1, C)).permute(0, 3, 1, 2)
    pds = (k["dyd"].float().permute(0, 2, 3, 1) @ k["wd"].float().view(Kd, C)).permute(0, 3, 1, 2)
    assert torch.equal(p1.double(), k["p1"]) and torch.equal(pds.double(), k["pds"])
    t = p1.to(BF16)
    t[:, :, ::2, ::2] = (t[:, :, ::2, ::2].float() + pds.to(BF16).float()).to(BF16)
    assert torch.equal(t, comp)
    assert torch.equal((p1 + zero_fill(pds.to(BF16).float(), H, W)).to(BF16), one)
    # the declined 14 x 14 case is the one-rounding contract as well
    k14 = ds_case(*DS_CASES["declined-14x14"][0])
    d14 = share(ds_expect(k14["p1"], k14["pds"], True)[:, :, ::2, ::2] != ds_expect(k14["p1"], k14["pds"], False, "dgrad")[:, :, ::2, ::2])
    assert d14 >= DIFFER_MIN


# ---------------------------------------------------------------------------------------------
# (b) a faithful fp32 emulation passes; the checkers reject perturbed results
# ---------------------------------------------------------------------------------------------
def bn_emulation(M=192, C=16, t=64, seed=1):
    """x, partials, and an fp32 BatchNorm (+ residual + ReLU) forward and backward as the kernels compute
    them, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, C, generator=g) * 1.5 + torch.randn(C, generator=g)).to(BF16)
    res = torch.randn(M, C, generator=g).to(BF16)
    w, b = torch.rand(C, generator=g) + 0.5, 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(M, C, generator=g).to(BF16)
    part = bk.tile_partials(x.double(), t)
    mean = part[:, 0].sum(0) / M
    tm = part[:, 0] / t
    var = (part[:, 1] + t * (tm - mean) ** 2).sum(0) / M
    invstd = (var + EPS).rsqrt()
    sc = w * invstd
    y = (x.float() * sc + (b - mean * sc) + res.float()).clamp_min(0).to(BF16)
    return dict(M=M, C=C, t=t, x=x, res=res, w=w, b=b, dy=dy, part=part, mean=mean, invstd=invstd, y=y)


def bn_bwd_fp32(g, x, mean, invstd, w):
    M = x.shape[0]
    xc = x.float() - mean
    s1, s2 = g.sum(0), (g * xc).sum(0)
    dg = s2 * invstd
    k = w * invstd
    return (k * g - k * s1 / M - (k * invstd * dg / M) * xc).to(BF16), dg, s1


def test_bn_emulation_passes_and_perturbations_fail():
    e = bn_emulation()
    M, C, t = e["M"], e["C"], e["t"]
    x64, w64, b64 = e["x"].double(), e["w"].double(), e["b"].double()
    mean_t, var_t, e_mean, e_var, L = tiles_stats(e["part"], t, M)
    assert L <= L_MAX and LT + chain_rows(M // t, True) <= L_MAX and chain_stats(M, C, True) <= L_MAX
    rep = Report("emulated forward")
    ref, _ = check_fwd_given(rep, "", x64, w64, b64, EPS, True, e["y"], e["mean"], e["invstd"], mean_t, var_t, e_mean, e_var,
                             e["res"].double(), 0.0)
    rep.check()
    rep = Report("float64 reference alone")
    check_fwd_given(rep, "", x64, w64, b64, EPS, True, ref["y"].to(BF16), mean_t.float(), ref["invstd"].float(), mean_t, var_t,
                    e_mean, e_var, e["res"].double(), 0.0)
    rep.check()
    assert max(r for _, r in rep.rows) <= 1.0
    # one dropped pixel of y
    rep = Report("dropped pixel")
    ybad = e["y"].clone()
    row = int((e["y"].float().abs().sum(1) > 1).nonzero()[0])
    ybad[row] = 0
    check_fwd_given(rep, "", x64, w64, b64, EPS, True, ybad, e["mean"], e["invstd"], mean_t, var_t, e_mean, e_var,
                    e["res"].double(), 0.0)
    rejects(rep.check)
    # backward
    ypos = e["y"] > 0
    g = e["dy"].float() * ypos
    dx, dg, db = bn_bwd_fp32(g, e["x"], e["mean"], e["invstd"], e["w"])
    dres = torch.where(ypos, e["dy"], torch.zeros_like(e["dy"]))
    N, H, W = 1, 1, M
    n4 = lambda r: bk.nhwc(r, N, H, W)
    g64, xc = g.double(), x64 - e["mean"].double()

    def run(out, gref=g64, L=chain_stats(M, C, True), want_dres=True, part=False):
        rep = Report("emulated backward")
        sums = bk.bwd_sums(gref, xc, L, exact_s1=False)
        if part:
            Lp = LT + chain_rows(M // t, True)
            sums = (gref.sum(0), (gref * xc).sum(0), Lp * U * gref.abs().sum(0), (Lp + 2) * U * (gref * xc).abs().sum(0))
        check_bwd(rep, "", out, gref, x64, e["mean"], e["invstd"], w64, L, want_dres, sums=sums)
        rep.check()

    run((n4(dx), n4(dres), dg, db))
    run((n4(dx), n4(dres), dg, db), part=True)
    ref_dx, ref_dg, ref_db = bn_bwd_ref(g64, x64, e["mean"].double(), e["invstd"].double(), w64)
    run((n4(ref_dx.to(BF16)), n4(dres), ref_dg.float(), ref_db.float()))             # the reference alone
    rejects(run, (n4(dres), n4(dx), dg, db))                                         # dx and dres swapped
    rejects(run, (n4(dx), n4(e["dy"]), dg, db))                                      # dres not masked
    # mask applied twice, where the contract hands dy on unmasked: the link check compares with dy itself
    assert not bk.same_bits(dres, e["dy"])
    # partials of the wrong tensor: the BatchNorm used dx1 alone although it received dx1 + dx2
    g2 = torch.randn(M, C, generator=torch.Generator().manual_seed(2)).to(BF16).float() * ypos
    both = (g + g2).to(BF16).float()
    dx_b, dg_b, db_b = bn_bwd_fp32(both, e["x"], e["mean"], e["invstd"], e["w"])
    run((n4(dx_b), None, dg_b, db_b), gref=both.double(), want_dres=False)
    rejects(run, (n4(dx), None, dg, db), gref=both.double(), want_dres=False)
    rejects(run, (n4(dx_b), None, dg, db_b), gref=both.double(), want_dres=False)    # only dgamma from the wrong sums


def test_conv_band_holds_for_fp32_and_rejects_a_dropped_pixel():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 64, 5, 6, generator=g).to(BF16)
    w = (torch.randn(128, 64, 3, 3, generator=g) / 24).to(BF16)
    ref, e = conv_bound(x, w, 1, 9 * 64)
    got = F.conv2d(x.float(), w.float(), padding=1).to(BF16)
    rep = Report("fp32 convolution")
    rep.add("y", got, ref, out_bound(ref, e))
    rep.add("float64 alone", ref.to(BF16), ref, out_bound(ref, e))
    rep.check()
    bad = got.clone()
    bad[1, :, 2, 3] = 0
    rep = Report("dropped pixel")
    rep.add("y", bad, ref, out_bound(ref, e))
    rejects(rep.check)


def test_bit_checks_reject_wiring_mistakes():
    """On the grid: one dropped pixel, the mask shifted by one byte, applied twice to a twice-masked
    expectation's neighbour (not applied), the compact add at transposed pixels, an arena overwrite, a
    doubled write and a write to the wrong slice — each reported at its first element in (n, h, w, c)."""
    name = "t256-k64-mask-arena"
    shape, alias, arena, route, want = CONV_NODE[name]
    N, C, H, W, K, R, st = shape
    e = conv_node_expect(name)
    c = e["c"]
    good = e["dx"]
    check_bits(nhwc(good.clone()), nhwc(good), NHWC, "identical")
    bad = good.clone()
    bad[2, :, 3, 5] = 0
    msg = first_mismatch(nhwc(bad), nhwc(good), NHWC)
    assert msg is not None and "n 2, h 3, w 5, channel" in msg
    rejects(check_bits, nhwc(bad), nhwc(good), NHWC, "dropped pixel")
    # the mask shifted by one byte
    bits = pack_mask(e["keep"])
    shifted = unpack_mask(torch.roll(bits, 1), N * H * W, C).view(N, H, W, C).permute(0, 3, 1, 2)
    rejects(check_bits, nhwc(dx_expect(c["dx"], c["add"] * shifted, route, K)), nhwc(good), NHWC, "shifted mask")
    # the mask not applied
    rejects(check_bits, nhwc(dx_expect(c["dx"], c["add"], route, K)), nhwc(good), NHWC, "mask not applied")
    # masked with a second, different mask on top (the residual BatchNorm masked as well, with its neighbour's bits)
    rejects(check_bits, nhwc(dx_expect(c["dx"], c["add"] * e["keep"] * shifted, route, K)), nhwc(good), NHWC, "masked twice")
    # the compact add at (2b, 2a): the compact tensor read with its two spatial axes exchanged
    dims = DS_CASES["compact-16x32"][0]
    k = ds_case(*dims)
    comp = ds_expect(k["p1"], k["pds"], True)
    Ho, Wo = k["pds"].shape[2:]
    assert Ho != Wo
    swapped = k["pds"].transpose(2, 3).reshape(k["pds"].shape)
    rejects(check_bits, nhwc(ds_expect(k["p1"], swapped, True)), nhwc(comp), NHWC, "compact add transposed")
    rejects(check_bits, nhwc(rne_bf16(k["p1"])), nhwc(comp), NHWC, "compact part dropped")
    # the arena: base + dW expected
    base, dw = c["base"], e["dw"]
    wantw = exact_f32(base + dw)
    check_bits(nhwc(exact_f32(base + dw)), nhwc(wantw), KRSC, "accumulated")
    rejects(check_bits, nhwc(exact_f32(dw)), nhwc(wantw), KRSC, "overwrite")
    rejects(check_bits, nhwc(exact_f32(base + 2 * dw)), nhwc(wantw), KRSC, "doubled write")
    n = wantw.numel()
    arena_want = torch.cat([torch.full((24,), 0.25), wantw.reshape(-1), torch.full((40,), 0.25)])
    arena_got = torch.cat([torch.full((16,), 0.25), wantw.reshape(-1), torch.full((48,), 0.25)])
    assert arena_got.numel() == arena_want.numel() == n + 64
    rejects(check_bits, arena_got, arena_want, ("arena element",), "wrong slice")
    # gamma = 0: dbeta from the unmasked gradient is another integer
    ki = ident_case("gemm-T256")
    assert not torch.equal(ki["g"].sum((0, 2, 3)), ki["dyo"].sum((0, 2, 3)))
    yo, keep = relu_res_expect(ki["beta"], ki["c"]["x"])
    assert torch.equal(keep, ki["keep"]) and torch.equal(yo, ki["yo"])
    assert torch.equal(stride2_add_ref(k["p1"] * 0, k["pds"] * 0), torch.zeros_like(comp))
    assert BIG * BIG * max(dims[4], dims[5]) < cx.LIM
