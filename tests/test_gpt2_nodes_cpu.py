"""CPU self-checks of what test_gpt2_nodes_gpu.py holds the GPT-2 autograd nodes to: the route helpers
and hooks, the grid cases' exactness preconditions and the share of elements in which the one-rounding
and two-rounding residual forms differ, the sparse gradients that keep a split dW exact, the float64
references and propagated bands (a faithful fp32 emulation passes, the reference alone stays inside
WIDE_CAP), and the checkers on perturbed references: one dropped row, a doubled bias, a swapped
dx / dr, a wrong accumulate — each must fail."""
import pytest
import torch

import test_gemm_nt_exact_gpu as ng
import test_gpt2_nodes_gpu as gn
import test_ln_gelu_embed_gpu as lg
from test_gemm_dw_exact_gpu import check_bits, first_mismatch
from test_gemm_nt_exact_gpu import A_MAX, DELTA, as_bf16, classify, rne
from test_gpt2_nodes_gpu import (C, F64, HID, LM_N, SPARSE_NNZ, V, VP, behind, either, forward_expect, grad_ints, grid,
                                 gints, linear_expect, ln_case_of, lm_case, lm_reference, mlp_backward_reference,
                                 mlp_cases, mlp_forward_reference, route_ok, stored_band)
from test_ln_gelu_embed_gpu import WIDE_CAP, check_banded, check_colgrad, ln_bwd_reference, randn16, share_ok, wide_count

BF16 = torch.bfloat16
DIFFER_MIN = 0.05   # share of elements in which two contracts must differ for a test to tell them apart
BAND_MAX = 0.10     # share of activation outputs inside the ambiguity band


def record(line):
    print(f"[nodes-cpu] {line}")


def share(mask):
    return float(mask.double().mean())


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ---------------------------------------------------------------------------------------------
# routes and hooks
# ---------------------------------------------------------------------------------------------
def test_route_helpers_and_hooks():
    x = torch.ones(3, requires_grad=True)
    y = (x * 2).exp().sum()
    names = gn.nodes(y)
    assert {"SumBackward0", "ExpBackward0", "MulBackward0", "AccumulateGrad"} <= names
    assert gn.producer(y.grad_fn) == "ExpBackward0"
    assert route_ok({"_LNResFnBackward", "_LinearResFnBackward"}, ["_LNResFn", "_LinearResFn"], ["_LinearFn"])
    assert not route_ok({"_LNResFnBackward", "_LinearFnBackward"}, ["_LNResFn"], ["_LinearFn"])
    assert not route_ok({"_LNResFnBackward"}, ["_LNResFn", "_LinearResFn"])
    rejects(gn.assert_route, y, ["_LinearFn"])           # a route that was not taken fails
    from paddle_operator_amd.ops import core, gpt2
    before = (gpt2._RES_EPI[0], core._NT_ALL[0], core._DW_CUS[0], gpt2._LM_CHUNK[0])
    with pytest.raises(RuntimeError):
        with gn.hooks(_RES_EPI=False, _NT_ALL=0, _DW_CUS=7, _LM_CHUNK=256):
            assert (gpt2._RES_EPI[0], core._NT_ALL[0], core._DW_CUS[0], gpt2._LM_CHUNK[0]) == (False, 0, 7, 256)
            raise RuntimeError("inside")
    assert (gpt2._RES_EPI[0], core._NT_ALL[0], core._DW_CUS[0], gpt2._LM_CHUNK[0]) == before
    for k in ("_RES_EPI", "_NT_GELU", "_NT_DGELU", "_NT_GD", "_NT_ALL", "_DX_TN", "_HIP_DW", "_QKV_FUSED", "_LM_CHUNK",
              "_XENT_FUSED", "_DW_GROUPED", "_DW_CUS"):
        with gn.hooks(**{k: 0}):
            pass
    # every route of the tables names node classes that exist
    have = set(dir(core)) | set(dir(gpt2))
    for table in (gn.RES_ROUTES, gn.MLP_ROUTES, gn.BLOCK_ROUTES):
        for entry in table.values():
            hk, lists = entry[0], entry[-2:]
            assert all(n in have for lst in lists for n in lst) and all(h in have for h in hk)
    for _, hk, _, ran, not_ran in gn.LM_ROUTES:
        assert all(n in have for n in ran + not_ran) and all(h in have for h in hk)


# ---------------------------------------------------------------------------------------------
# (a) the grid cases
# ---------------------------------------------------------------------------------------------
def test_k128_residual_case_takes_the_two_rounding_form():
    """K = 128 is outside _res_epi_ok (K >= 256): the case's expected h is the two-rounding form, which
    differs from the epilogue's one rounding in a useful share, so a residual epilogue on the ring would show."""
    c = grid(256, C, 128)
    fw = forward_expect(c)
    assert c["K"] == 128 and gn.RES_K["k128"] == 128 and gn.RES_ROUTES["k128"][2] == ["_LinearFn", "_AddLayerNormFn"]
    assert share(fw["h_fused"] != fw["h_unfused"]) >= DIFFER_MIN
    for v in fw.values():
        as_bf16(v * c["u"])


@pytest.mark.parametrize("T", (256, 768))
def test_grid_cases_exact_and_contracts_distinguishable(T):
    """Operands bf16-exact, every sum below 2^24 (the builders assert it), and the fused (one rounding)
    and unfused (two) residual forms differ in at least 5 % of the elements, as do EPI 1 and a bias
    added after the rounding."""
    c = grid(T, C, C)
    u, fw = c["u"], forward_expect(c)
    for t in (c["a"], c["b"] * u, c["bias"] * u, ng.addend(c) * u):
        as_bf16(t)
    for v in fw.values():
        as_bf16(v * u)
    d_h, d_y = share(fw["h_fused"] != fw["h_unfused"]), share(fw["y"] != fw["y_two"])
    record(f"T={T}: fused and unfused h differ in {d_h:.1%}, one- and two-rounding y in {d_y:.1%}")
    assert d_h >= DIFFER_MIN and d_y >= DIFFER_MIN
    dy = grad_ints(T, C, 11 + T)
    e = linear_expect(c, dy)
    for k in ("dx", "dw", "db"):
        as_bf16(e[k] * (u if k == "dx" else 1.0))
    if T == 256:   # dense: most exact dW values need a rounding (the sparse ones are bf16-exact by design)
        assert share(rne(dy.t() @ c["a"]) != dy.t() @ c["a"]) > 0.3


def test_sparse_gradient_keeps_any_split_exact():
    """grad_ints beyond T = 256: SPARSE_NNZ entries of +-1 per column, every row occupied, so every
    partial sum over any token subset is at most 240 and bf16-exact; the split-and-round emulation of
    gemm_dw then equals RNE(base + exact) for every split of the token axis."""
    T = 768
    dy, c = grad_ints(T, C, 5), grid(T, C, C)
    assert int((dy != 0).sum(0).max()) == SPARSE_NNZ and float(dy.abs().max()) == 1.0
    assert bool((dy != 0).any(1).all()) and SPARSE_NNZ * A_MAX <= 256
    base = gints((C, C), 6, 255)
    exact = dy.t() @ c["a"]
    for cuts in ((0, 768), (0, 256, 512, 768), (0, 320, 768), (0, 64, 128, 704, 768)):
        parts = [rne(dy[a:b].t() @ c["a"][a:b]) for a, b in zip(cuts, cuts[1:])]
        assert torch.equal(rne(base + sum(parts)), rne(base + exact))
    dense = gints((T, C), 7)
    parts = [rne(dense[a:b].t() @ c["a"][a:b]) for a, b in ((0, 256), (256, 512), (512, 768))]
    assert share(rne(sum(parts)) != rne(dense.t() @ c["a"])) > 0.01   # a dense gradient would not be exact


def test_checkers_reject_a_dropped_row():
    """One token row missing from dW, db and drbias; one 128-row partial missing from db: check_bits fails."""
    for T in (256, 768):
        c = grid(T, C, C)
        dy = grad_ints(T, C, 11 + T)
        e = linear_expect(c, dy)
        row = T // 2 + 3
        assert bool((dy[row] != 0).any())
        cut = dy.clone()
        cut[row] = 0.0
        bad = linear_expect(c, cut)
        for k in ("dw", "db"):
            assert first_mismatch(as_bf16(bad[k]).reshape(-1, C), as_bf16(e[k]).reshape(-1, C)) is not None, (T, k)
        rejects(check_bits, as_bf16(bad["dw"]), as_bf16(e["dw"]), "dW without one row")
        twice = dy.clone()
        twice[row] *= 2.0
        assert first_mismatch(as_bf16(rne(twice.t() @ c["a"])), as_bf16(e["dw"])) is not None
        part = dy.clone()
        part[128:256] = 0.0
        assert first_mismatch(as_bf16(rne(part.sum(0))).view(1, -1), as_bf16(e["db"]).view(1, -1)) is not None
    # the forward: a row of h taken from its neighbour
    fw = forward_expect(grid(256, C, C))
    moved = fw["h_fused"].clone()
    moved[17] = fw["h_fused"][18]
    rejects(check_bits, as_bf16(moved), as_bf16(fw["h_fused"]), "h with a displaced row")


def test_checkers_reject_a_doubled_bias():
    """The bias added in the GEMM epilogue and again in the LayerNorm kernel: h changes bits, and the
    LayerNorm's y of the doubled h falls outside the bands of the reference."""
    c = grid(256, C, C)
    u, fw = c["u"], forward_expect(c)
    doubled = rne(c["p"] + 2.0 * c["bias"] + ng.addend(c))
    assert share(doubled != fw["h_fused"]) > 0.5
    rejects(check_bits, as_bf16(doubled * u), as_bf16(fw["h_fused"] * u), "h with the bias twice")
    rejects(either, as_bf16(rne(c["p"] + 2.0 * c["bias"]) * u), [as_bf16(fw["y"] * u), as_bf16(fw["y_two"] * u)], "y")
    either(as_bf16(fw["y_two"] * u), [as_bf16(fw["y"] * u), as_bf16(fw["y_two"] * u)], "the library's two roundings")
    gen = torch.Generator().manual_seed(3)
    w, b = randn16((C,), gen), randn16((C,), gen)
    lc = ln_case_of((fw["h_fused"] * u).to(torch.float32), w, b)
    check_banded(as_bf16(rne(lc["y"])), lc["y"], lc["band"], "y of the reference itself", wide_cap=WIDE_CAP)
    y2 = ln_case_of((doubled * u).to(torch.float32), w, b)["y"]
    rejects(check_banded, as_bf16(rne(y2)), lc["y"], lc["band"], "y of the doubled h")
    # drbias summed over the rounded dx twice
    db = rne(gints((256, C), 9).sum(0))
    rejects(check_bits, as_bf16(2.0 * db).view(1, -1), as_bf16(db).view(1, -1), "drbias twice")


def test_checkers_reject_swapped_gradients():
    """dx for dr (the unmasked for the masked stream), and dh for dy in the LayerNorm backward."""
    T = 256
    keep = (torch.rand(T, C, generator=torch.Generator().manual_seed(4)) < 0.5).to(F64)
    g1 = gints((T, C), 82)
    dx, dr = as_bf16(g1), as_bf16(2.0 * keep * g1)
    rejects(check_bits, dr, dx, "dx returned as dr")
    rejects(check_bits, dx, dr, "dr returned as dx")
    assert share(rne((2.0 * keep * g1).sum(0)) != rne(g1.sum(0))) > 0.9          # drbias of the wrong stream
    gen = torch.Generator().manual_seed(5)
    h, w, g2, gr = randn16((T, C), gen), randn16((C,), gen), randn16((T, C), gen), randn16((T, C), gen)
    mu = h.mean(1)
    rs = 1.0 / torch.sqrt(((h - mu[:, None]) ** 2).mean(1) + lg.EPS)
    ref = ln_bwd_reference(h, g2, w, mu, rs, gr)
    check_banded(as_bf16(rne(ref["dx"])), ref["dx"], ref["band"], "dx of the reference itself", wide_cap=WIDE_CAP)
    swapped = ln_bwd_reference(h, gr, w, mu, rs, g2)
    rejects(check_banded, as_bf16(rne(swapped["dx"])), ref["dx"], ref["band"], "dh and dy swapped")
    for name in ("dgamma", "dbeta", "drbias"):
        check_colgrad(name, as_bf16(rne(ref[name][0])), ref, "the reference itself")
        rejects(check_colgrad, name, as_bf16(rne(swapped[name][0])), ref, "swapped")
    # one row dropped from a column gradient
    cut = g2.clone()
    cut[100] = 0.0
    rejects(check_colgrad, "dbeta", as_bf16(rne(cut.sum(0))), ref, "dbeta without a row")


def test_checkers_reject_a_wrong_accumulate():
    """accumulate clear on the second micro-batch (the second alone) and a base added twice."""
    for T in (256, 768):
        c = grid(T, C, C)
        dy1, dy2, a2 = grad_ints(T, C, 11 + T), grad_ints(T, C, 12 + T), gints((T, C), 13 + T, A_MAX)
        e1 = linear_expect(c, dy1)
        e2 = linear_expect(c, dy2, a2, prev=dict(w=e1["dw"], b=e1["db"]))
        alone = linear_expect(c, dy2, a2)
        for k in ("dw", "db"):
            assert share(alone[k] != e2[k]) > 0.5, (T, k)
            rejects(check_bits, as_bf16(alone[k]).reshape(-1, C), as_bf16(e2[k]).reshape(-1, C), "the second alone")
            twice = rne(2.0 * e1[k] + (e2[k] - e1[k]))
            assert first_mismatch(as_bf16(twice).reshape(-1, C), as_bf16(e2[k]).reshape(-1, C)) is not None
        # the rounding of the first backward is part of the contract: RNE(RNE(first) + second)
        if T == 256:
            once = rne(dy1.t() @ c["a"] + dy2.t() @ a2)
            assert share(once != e2["dw"]) > 0.01
        either(as_bf16(e2["two"]["dw"]), [as_bf16(e2["dw"]), as_bf16(e2["two"]["dw"])], "library accumulate")
        rejects(either, as_bf16(alone["dw"]), [as_bf16(e2["dw"]), as_bf16(e2["two"]["dw"])], "the second alone")
    # accum_ok with another second micro-batch: alone = RNE(s2), second = RNE(first + s2)
    s1 = torch.randn(4096, generator=torch.Generator().manual_seed(7), dtype=F64) * 3.0
    s2 = torch.randn(4096, generator=torch.Generator().manual_seed(8), dtype=F64) * 3.0
    f1, alone2 = as_bf16(rne(s1)), as_bf16(rne(s2))
    assert bool(gn.accum_ok(f1, as_bf16(rne(rne(s1) + s2)), alone2).all())
    assert share(gn.accum_ok(f1, alone2, alone2)) < 0.01                         # accumulate clear on the second
    assert share(gn.accum_ok(f1, as_bf16(rne(2.0 * rne(s1))), alone2)) < 0.01    # the first micro-batch again
    assert share(gn.accum_ok(f1, as_bf16(rne(2.0 * rne(s1) + s2)), alone2)) < 0.01   # the base added twice
    # accum_ok: inexact sums s, first = RNE(s), second = RNE(first + s)
    s = torch.randn(4096, generator=torch.Generator().manual_seed(6), dtype=F64) * 3.0
    first = rne(s)
    assert bool(gn.accum_ok(as_bf16(first), as_bf16(rne(first + s))).all())
    assert share(gn.accum_ok(as_bf16(first), as_bf16(first))) < 0.001            # accumulate clear: the sum alone
    assert share(gn.accum_ok(as_bf16(first), as_bf16(rne(3.0 * s)))) < 0.001      # the base added twice


# ---------------------------------------------------------------------------------------------
# (b) references and bands
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (256, 768))
@pytest.mark.parametrize("fused", (True, False))
def test_residual_layernorm_references_stay_inside_the_wide_cap(T, fused):
    c = grid(T, C, C)
    u, fw = c["u"], forward_expect(c)
    gen = torch.Generator().manual_seed(71 + T)
    lnw, lnb, g1, g2 = (randn16(s, gen) for s in ((C,), (C,), (T, C), (T, C)))
    v = (fw["h_fused"] if fused else ng.addend(c) + fw["plain"] + c["bias"]) * u
    assert torch.equal(v.to(torch.float32).to(F64), v)         # the fp32 row is exact
    lc = ln_case_of(v.to(torch.float32), lnw, lnb)
    n = v.numel()
    assert share_ok(wide_count(lc["y"], lc["band"]), n, WIDE_CAP)
    assert float((lg.k_rstd(C) + lc["extra"] + 4).max()) <= lg.k_y(C)
    h = rne(v)
    ref = ln_bwd_reference(h, g2, lnw, lc["mu"], lc["rstd"], g1)
    assert share_ok(wide_count(ref["dx"], ref["band"]), n, WIDE_CAP)
    record(f"T={T} fused={fused}: y band share {lg.band_share(lc['y'], lc['band']):.3%}, dx band share "
           f"{lg.band_share(ref['dx'], ref['band']):.3%}")


def test_behind_bounds_an_fp32_gemm_and_rejects_a_dropped_slice():
    gen = torch.Generator().manual_seed(8)
    a, b = randn16((64, 512), gen), randn16((512, 96), gen)
    ref, band = behind(a, None, b, 512)
    got = (a.to(torch.float32) @ b.to(torch.float32)).to(BF16)
    check_banded(got, ref, band, "fp32 GEMM")
    cut = a.clone()
    cut[:, 100:101] = 0.0
    rejects(check_banded, (cut.to(torch.float32) @ b.to(torch.float32)).to(BF16), ref, band, "one k index dropped")
    # a stored under the activation rule: float64 values v, stored as RNE(v), or as either neighbour
    # where v lies inside the ambiguity band of a midpoint — each within stored_band(v), and the GEMM of
    # the stored values inside the propagated band
    v = a * (1.0 + 2.0 ** -9 * torch.rand(a.shape, generator=gen, dtype=F64))
    lo, hi, near, _ = classify(v)
    assert bool(((near - v).abs() <= stored_band(v)).all())
    check_banded((near.to(torch.float32) @ b.to(torch.float32)).to(BF16), *behind(v, stored_band(v), b, 512), "RNE(v)")
    mid = 0.5 * (lo + hi) * (1.0 + 0.5 * DELTA)
    assert bool(classify(mid)[3][lo != hi].all())
    ref2, band2 = behind(mid, stored_band(mid), b, 512)
    for other in (lo, hi):
        assert bool(((other - mid).abs() <= stored_band(mid)).all())
        check_banded((other.to(torch.float32) @ b.to(torch.float32)).to(BF16), ref2, band2, "a neighbour in the band")
    # the split form: partials rounded to bf16, then folded
    parts = [(a[:, k:k + 128].to(torch.float32) @ b[k:k + 128].to(torch.float32)).to(BF16).to(torch.float32)
             for k in range(0, 512, 128)]
    check_banded(sum(parts).to(BF16), *behind(a, None, b, 512, True), "split GEMM")


@pytest.mark.parametrize("T", (256, 768))
def test_mlp_references(T):
    """Argument range, band shares, the fused and unfused GELU arguments give different bits in a
    useful share, and a faithful fp32 emulation of each backward route stays inside its bands while a
    dropped row does not — with the bands the GPU test uses at that T: at T = 768 gemm_dw splits the
    token axis and the dW bands carry the bf16 partials' 2^-8 sum |terms|."""
    c1, c2 = mlp_cases(T)
    fr, un = mlp_forward_reference(c1, True), mlp_forward_reference(c1, False)
    for name in ("h", "gd"):
        assert share(classify(fr[name])[3]) <= BAND_MAX
    assert 1.0 <= float(fr["arg"].std()) <= 2.5       # the spread test_gemm_nt_exact_cpu.py asks of a GELU argument
    d = share(rne(fr["h"]) != rne(un["h"]))
    record(f"T={T}: fused (one rounding) and unfused (two) gelu outputs differ in {d:.1%}")
    assert d >= DIFFER_MIN
    g = gints((T, C), 91 + T)
    h, f32 = rne(fr["h"]), torch.float32
    w1, w2, x = c1["b"] * c1["u"], c2["b"] * c2["u"], c1["a"]
    p2 = g @ w2
    split = T > 256     # gemm_dw_splits(768, ...) = 3 (ks = 12 k-tiles allow 3 slices); one split at T = 256
    for route, saved in (("saved", rne(fr["gd"])), ("recompute", fr["hp"]), ("bias_gelu", fr["hp"])):
        refs = mlp_backward_reference(route, c1, c2, h, saved, g, split)
        if route == "saved":
            d32 = p2.to(f32) * saved.to(f32)
        else:
            arg = lg.gelu_arg(saved, c1["gbias"])
            lhs = rne(p2) if route == "bias_gelu" else p2
            d32 = (lhs * ng.gelu_grad64(arg)).to(f32)
        dhp = d32.to(BF16)                      # the kernels sum the unrounded fp32 d into db1
        emu = dict(dx=(dhp.to(f32) @ w1.to(f32)).to(BF16), dw1=(dhp.to(f32).t() @ x.to(f32)).to(BF16),
                   dw2=(g.to(f32).t() @ h.to(f32)).to(BF16))
        for n, t in emu.items():
            check_banded(t, refs[n][0], refs[n][1], f"{route} {n}")
        s, bound = refs["db1"]
        assert bool(((rne(d32.sum(0).double()) - s).abs() <= bound).all())
        cut = dhp.clone()
        cut[T // 2] = 0.0
        rejects(check_banded, (cut.to(f32).t() @ x.to(f32)).to(BF16), refs["dw1"][0], refs["dw1"][1], "dW1 without a row")
    # the saved-gelu' route multiplies by the STORED derivative: the recomputed one is refused
    refs = mlp_backward_reference("saved", c1, c2, h, rne(fr["gd"]), g, split)
    other = as_bf16(rne(p2 * ng.gelu_grad64(fr["hp"] + c1["gbias"])))
    rejects(check_banded, (other.to(f32) @ w1.to(f32)).to(BF16), refs["dx"][0], refs["dx"][1], "dx of the other route")
    assert HID == c1["N"] and C == c2["N"]


def emulate_lm(ref_d, k, chunks=1):
    """A faithful LM head on the CPU: dlogits rounded to bf16, fp32 GEMMs, dW accumulated per chunk."""
    c = k["c"]
    f32 = torch.float32
    dl = ref_d.to(f32).to(BF16).to(f32)
    w, h = (c["b"] * c["u"]).to(f32), c["a"].to(f32)
    dw = torch.zeros(VP, C, dtype=f32)
    for rows in torch.arange(LM_N).chunk(chunks):
        dw = (dw + dl[rows].t() @ h[rows]).to(BF16).to(f32)
    return dict(dh=(dl @ w).to(BF16), dw=dw.to(BF16))


def test_lm_head_reference_and_checker():
    """The targets hold -100, V, Vp - 1 and -1, all in the first chunk, and one more ignored target in
    the second; a faithful emulation passes at one and two chunks; a gradient for an ignored token, a
    padding row in dW, a per-chunk count and a dropped token row are each rejected."""
    from test_small_kernels_gpu import xent_ref
    k = lm_case()
    tgt = k["tgt"]
    assert {-100, V, VP - 1, -1} <= set(tgt[:256].tolist()) and int(k["dead"][256:].sum()) == 1
    assert int(k["dead"].sum()) == 5 and VP - V == 84
    loss, _, d, cnt = xent_ref(k["logits"], tgt, V, 1.0)
    for chunks in (1, 2):
        ref = lm_reference(1.0, chunks, chunks == 1)
        r = dict(loss=loss, **emulate_lm(d, k, chunks))
        gn.check_lm(r, ref, f"emulated LM head, {chunks} chunk(s)")
    ref = lm_reference(1.0, 1, True)      # the band of the GPU test: gemm_dw splits N = 512 in two
    good = dict(loss=loss, **emulate_lm(d, k))
    bad = dict(good, dh=good["dh"].clone())
    bad["dh"][3] = good["dh"][4]
    rejects(gn.check_lm, bad, ref, "an ignored token with a gradient")
    bad = dict(good, dw=good["dw"].clone())
    bad["dw"][V + 1] = good["dw"][0]
    rejects(gn.check_lm, bad, ref, "a padding row with a gradient")
    per_chunk = d.clone()
    per_chunk[:256] *= cnt / float((~k["dead"][:256]).sum())
    per_chunk[256:] *= cnt / float((~k["dead"][256:]).sum())
    rejects(gn.check_lm, dict(loss=loss, **emulate_lm(per_chunk, k)), ref, "a per-chunk count")
    rejects(gn.check_lm, dict(good, loss=loss * 507.0 / 252.0), ref, "the loss of a per-chunk count")
    cut = d.clone()
    cut[5] = 0.0
    rejects(gn.check_lm, dict(loss=loss, **emulate_lm(cut, k)), ref, "a dropped token row")
    half = lm_reference(0.5)
    assert torch.equal(half["dh"], 0.5 * ref["dh"]) and torch.equal(half["dw"], 0.5 * ref["dw"])


def test_embedding_case_crosses_segments_and_dropout_scale():
    k = gn.embed_case()
    idx = k["idx"].flatten()
    assert int(idx.min()) >= 0 and int(idx.max()) < VP     # the forward reads wte[idx]: in range
    keys = torch.sort(idx, stable=True)[0].tolist()
    crossing = [t for t in set(keys) if keys.index(t) // 256 != (len(keys) - 1 - keys[::-1].index(t)) // 256]
    assert crossing, "no run of equal ids crosses a 256-row segment"
    assert int(torch.bincount(idx, minlength=VP).max()) > 256
    spec = gn.half_spec()
    keep = gn.keep_mask((256, C), spec)
    assert 0.45 < float(keep.mean()) < 0.55 and spec.scale == 2.0
