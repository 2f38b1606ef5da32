"""CPU checks of the builders, references and checkers of test_ln_gelu_embed_gpu.py: the float64
references against torch's own operators and autograd, the preconditions the GPU tests rely on (band
shares, the counted constants, the id patterns, the sweep tensor), and sensitivity: each checker must
accept outputs rounded from the reference and reject outputs rounded from a perturbed one."""
import pytest
import torch
import torch.nn.functional as F

import test_ln_gelu_embed_gpu as t
from test_gemm_nt_exact_gpu import as_bf16, check_activation, classify, gelu64, gelu_grad64, rne

BF16 = torch.bfloat16
F64 = torch.float64
ALL_LN = [(N, C, form, False) for N, C, _ in t.LN_FWD for form in t.LN_FORMS] + \
         [(t.ADV_N, C, form, True) for C in t.LN_ADV_C for form in ("plain", "add")]


def _id(case):
    N, C, form, adv = case
    return f"{N}x{C}-{form}{'-adv' if adv else ''}"


def as_kernel_outputs(ref):
    """What a faultless kernel would return for a reference: fp32 mean / rstd, y rounded once."""
    return ref["mu"].to(torch.float32), ref["rstd"].to(torch.float32), as_bf16(rne(ref["y"]))


# ---------------------------------------------------------------------------------------------
# references against torch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", [(5, 520), (37, 776), (3, 3080)])
def test_layernorm_references_match_torch_autograd(N, C):
    c = t.ln_case(N, C, "add_rbias")
    v = c["v32"].to(F64).requires_grad_(True)
    w, b = c["w"].clone().requires_grad_(True), c["b"].clone().requires_grad_(True)
    y = F.layer_norm(v, (C,), w, b, t.EPS)
    assert float((y.detach() - c["y"]).abs().max()) < 1e-12
    assert float((v.detach().mean(1) - c["mu"]).abs().max()) < 1e-14
    i = t.ln_bwd_inputs(N, C, False)
    y.backward(i["dy"])
    ref = t.ln_bwd_reference(c["v32"].to(F64), i["dy"], c["w"], c["mu"], c["rstd"], i["dres"])
    assert float((v.grad + i["dres"] - ref["dx"]).abs().max()) < 1e-11
    assert float((w.grad - ref["dgamma"][0]).abs().max()) < 1e-11
    assert float((b.grad - ref["dbeta"][0]).abs().max()) < 1e-11
    assert float(((v.grad + i["dres"]).sum(0) - ref["drbias"][0]).abs().max()) < 1e-11
    plain = t.ln_bwd_reference(c["v32"].to(F64), i["dy"], c["w"], c["mu"], c["rstd"], None)
    assert float((v.grad - plain["dx"]).abs().max()) < 1e-11


def test_gelu_references_match_torch_and_gelu64():
    x = torch.linspace(-8, 8, 4001, dtype=F64).requires_grad_(True)
    y = F.gelu(x, approximate="tanh")
    y.sum().backward()
    xd = x.detach()
    assert float((t.gelu_ref(xd) - y.detach()).abs().max()) < 1e-14
    assert float((t.gelu_grad_ref(xd) - x.grad).abs().max()) < 1e-14
    assert float((t.gelu_ref(xd) - gelu64(xd)).abs().max()) < 1e-14
    assert float((t.gelu_grad_ref(xd) - gelu_grad64(xd)).abs().max()) < 1e-14
    # why the logistic form: 1 + tanh(u) moves in steps of 2^-53, so the tanh form is percent-wrong at
    # x = -7 and exactly 0 from x = -7.5 on, for values of 1e-15 .. 1e-21 that the kernel resolves to
    # 2^-16 relative; the logistic form keeps its relative accuracy
    lo = torch.tensor([-7.0, -7.5, -8.0], dtype=F64)
    assert bool((gelu64(lo[1:]) == 0).all()) and bool((t.gelu_ref(lo) < 0).all())
    assert abs(float(gelu64(lo[:1]) / t.gelu_ref(lo[:1])) - 1.0) > 1e-3
    exact = lo * torch.exp(2.0 * t.GK0 * (lo + t.GK1 * lo ** 3))    # sigma(z) = e^z (1 - e^z + ...), e^z < 1e-17
    assert float(((t.gelu_ref(lo) - exact) / exact).abs().max()) < 1e-14
    # every finite bf16 argument gives a finite reference
    a = t.sweep_patterns().to(F64)
    assert bool(torch.isfinite(t.gelu_ref(a)).all()) and bool(torch.isfinite(t.gelu_grad_ref(a)).all())


# ---------------------------------------------------------------------------------------------
# preconditions of the GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_LN, ids=_id)
def test_layernorm_band_shares_and_counted_constants(case):
    """Random rows: at most 2 % of the elements lie in y's ambiguity band (one element in a case of
    fewer than 50) and at most 0.5 % have a band that spans more than two bf16 values; offset rows: at
    most 10 % and 5 % (OFFSET = 16 standard deviations).  For every row but the constant one, whose
    centred values are zero in the reference, the count K_RSTD + X + 4 of the module docstring stays
    within K_Y."""
    N, C, form, adv = case
    c = t.ln_case(N, C, form, adv)
    kinds = t.ADV_ROWS if adv else {}
    random_rows = [r for r in range(c["N"]) if r not in kinds]
    share = t.band_share(c["y"], c["band"], random_rows)
    n = len(random_rows) * C
    wide = t.wide_count(c["y"], c["band"], random_rows)
    print(f"[ln-gelu-embed] {_id(case)}: band share of the random rows {share:.3%}, more than two values "
          f"{wide / n:.3%}")
    assert t.share_ok(round(share * n), n, t.RANDOM_CAP)
    assert t.share_ok(wide, n, t.WIDE_CAP)
    for r, kind in kinds.items():
        s = t.band_share(c["y"], c["band"], [r])
        wide = t.wide_count(c["y"], c["band"], [r])
        print(f"[ln-gelu-embed] {_id(case)}: band share of the {kind} row {r}: {s:.3%}, more than two values "
              f"{wide / C:.3%}")
        if kind == "offset":
            assert s <= t.OFFSET_CAP and wide <= t.OFFSET_CAP / 2 * C
    rows = [r for r in range(c["N"]) if kinds.get(r) != "constant"]
    need = t.k_rstd(C) + c["extra"][rows] + 4
    assert float(need.max()) <= t.k_y(C), (float(need.max()), t.k_y(C))
    assert t.k_mean(C) <= t.k_y(C)


def test_layernorm_adversarial_rows_are_what_they_claim():
    for C in t.LN_ADV_C:
        x = t.ln_case(t.ADV_N, C, "plain", adv=True)["x"]
        for r, kind in t.ADV_ROWS.items():
            row = x[r]
            if kind == "offset":
                assert abs(float(row.mean())) > 12 * float(row.std())
            elif kind == "needle":
                assert int((row != 0).sum()) == 1
            elif kind == "constant":
                assert bool((row == t.CONST_VALUE).all())
            else:
                bits = as_bf16(row).view(torch.int16)
                assert set(bits.tolist()) == {int(bits.min()), int(bits.min()) + 1}


def test_vpl_and_backward_shapes_reach_their_paths():
    assert [t.vpl_for(C) for _, C, _ in t.LN_FWD] == [1, 1, 2, 2, 4, 4, 5, 6, 8, 8]
    assert all(t.vpl_for(C) <= 4 for _, C in t.LN_BWD) and t.vpl_for(2056) == 5
    grid = lambda N: max(1, min(512, (N + 15) // 16))  # noqa: E731  layernorm_bwd_grid
    assert grid(8197) == 512 and 8197 // (4 * 512) == 4 and 8197 % (4 * 512) == 5
    assert grid(1) == 1 and grid(5) == 1              # 3 of 4 waves have no row; 5 rows: wave 0 takes two


def test_gelu_shapes_reach_their_paths():
    def fwd(N, Fdim):   # bias_gelu_fwd's grid
        F8 = Fdim // 8
        nvec = N * F8
        per = F8 // 256 if F8 % 256 == 0 else F8
        g = max(1, 2048 // per) * per
        need = (nvec + 255) // 256
        if g > need:
            g = (need + per - 1) // per * per
        assert (g * 256) % F8 == 0
        return F8 % 256 == 0, g, nvec / (g * 256)
    assert fwd(3, 8) == (False, 1, 3 / 256)
    assert fwd(1100, 4096)[:2] == (True, 2048) and 1 < fwd(1100, 4096)[2] < 2
    assert fwd(4200, 1000)[:2] == (False, 2000) and 1 < fwd(4200, 1000)[2] < 2
    assert fwd(77, 3072)[:2] == (False, 384)

    def bwd(N, Fdim):   # (gx, gy, rows_per, first empty y-block or None)
        gx = (Fdim // 8 + 255) // 256
        gy = max(1, min(2048 // gx, N))
        rows_per = -(-N // gy)
        empty = -(-N // rows_per)
        return gx, gy, rows_per, empty if empty < gy else None
    assert bwd(5, 64) == (1, 5, 1, None)
    assert bwd(2049, 64) == (1, 2048, 2, 1025)
    assert bwd(8195, 8)[:3] == (1, 2048, 5)
    assert bwd(77, 3072)[:2] == (2, 77)
    for N, Fdim, _ in t.GELU_FWD + t.GELU_BWD:
        c = t.gelu_case(N, Fdim)
        assert float(t.gelu_arg(c["x"], c["b"]).abs().max()) <= t.X_LIMIT
        b = c["b"]
        assert all(float(b[i]) != float(b[(i + 8 * k) % Fdim]) for i in range(min(Fdim, 16)) for k in range(1, 24)
                   if (8 * k) % Fdim and (8 * k) % 193)


def test_sweep_holds_every_pattern():
    x = t.sweep_patterns()
    assert x.shape == (64, 1024) and x.dtype == BF16
    bits = set((x.view(torch.int16).to(torch.int32) & 0xFFFF).flatten().tolist())
    nonfinite = {p for p in range(65536) if (p & 0x7F80) == 0x7F80}
    assert len(nonfinite) == 256 and bits == set(range(65536)) - nonfinite | {0}
    assert int((x.view(torch.int16) == 0).sum()) == 257   # +0 itself and the replaced patterns


@pytest.mark.parametrize("name", sorted(t.PATTERNS))
def test_id_patterns_contain_their_run_kinds(name):
    B, S, idx = t.id_pattern(name)
    keys, perm = torch.sort(idx.flatten(), stable=True)
    assert t.run_kinds(keys, t.EMB_VP) == t.PATTERN_KINDS[name]
    assert not torch.equal(perm, torch.arange(B * S))
    assert int((keys < 0).sum()) >= 3
    if name == "785b":
        assert int((keys >= t.EMB_VP).sum()) >= 3
    union = set().union(*t.PATTERN_KINDS.values())
    assert len(union) == 10   # every situation run_kinds knows occurs in some pattern


# ---------------------------------------------------------------------------------------------
# the sorted-embedding reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(t.PATTERNS))
def test_sorted_reference_matches_float64_index_add(name):
    c = t.sorted_case(name, 64)
    N = c["B"] * c["S"]
    flat = c["idx"].flatten()
    ok = (flat >= 0) & (flat < t.EMB_VP)
    d = c["dy"].reshape(N, 64)
    ref = c["base"].to(F64).index_add_(0, flat[ok], d[ok])
    mass = c["base"].to(F64).abs().index_add_(0, flat[ok], d[ok].abs())
    # fp32 accumulation of at most N terms, then one bf16 rounding
    bound = N * t.U * mass + 2.0 ** -8 * ref.abs() + 1e-30
    assert bool(((c["want"].to(F64) - ref).abs() <= bound).all())
    untouched = [i for i in range(t.EMB_VP) if i not in set(flat[ok].tolist())]
    assert untouched and torch.equal(c["want"][untouched].view(torch.int16), c["base"][untouched].view(torch.int16))


def test_sorted_reference_follows_the_order():
    """Hand-worked: one id, rows 2^24, 1, -2^24.  fp32 in row order: 2^24 + 1 = 2^24 (tie to even),
    - 2^24 = 0; in the order 2^24, -2^24, 1 the sum is 1."""
    dy = torch.tensor([[2.0 ** 24] * 8, [1.0] * 8, [-2.0 ** 24] * 8])
    keys = torch.zeros(3, dtype=torch.int64)
    base = torch.zeros(2, 8, dtype=BF16)
    a = t.sorted_reference(dy, keys, torch.tensor([0, 1, 2]), base)
    b = t.sorted_reference(dy, keys, torch.tensor([0, 2, 1]), base)
    assert bool((a[0] == 0).all()) and bool((b[0] == 1).all()) and bool((a[1] == 0).all())


def test_sorted_reference_rejects_a_swap_across_a_segment_boundary():
    """Rows 255 and 256 of the sorted order carry the same id in pattern 785a (the run 50 .. 519);
    swapping them moves each into the other segment's piece.  After the bf16 rounding random columns
    rarely show that; the pinned columns (order_pins) do: column 0 turns from 0 into 1.  A reference
    that summed the run straight through, ignoring the pieces, differs in column 1."""
    c = t.sorted_case("785a", 520)
    N = c["B"] * c["S"]
    assert int(c["keys"][255]) == int(c["keys"][256]) == 3
    assert float(c["want"][3, 0]) == 0.0 and float(c["want"][3, 1]) == 1.0
    dy = c["dy"].reshape(N, 520).to(torch.float32)
    perm = c["perm"].clone()
    perm[[255, 256]] = perm[[256, 255]]
    swapped = t.sorted_reference(dy, c["keys"], perm, c["base"])
    assert float(swapped[3, 0]) == 1.0
    assert torch.equal(swapped[4].view(torch.int16), c["want"][4].view(torch.int16))   # other ids unaffected
    straight = torch.zeros(2, dtype=torch.float32)
    for j in range(50, 520):
        straight = straight + dy[c["perm"][j], :2]
    assert straight.tolist() == [0.0, 0.0]


# ---------------------------------------------------------------------------------------------
# sensitivity of the checkers
# ---------------------------------------------------------------------------------------------
def test_layernorm_checker_accepts_the_reference_and_rejects_one_ulp():
    c = t.ln_case(37, 776, "add_rbias")
    mean, rstd, y = as_kernel_outputs(c)
    h = c["v32"].to(BF16)
    t.check_ln_forward(c, mean, rstd, y, h, "reference outputs")
    _, _, _, amb = classify(c["y"], band=c["band"])
    k = int((~amb[20]).nonzero()[5])          # an element outside the band
    bad = y.clone()
    bad.view(torch.int16)[20, k] += 1         # one bf16 ulp
    with pytest.raises(AssertionError):
        t.check_ln_forward(c, mean, rstd, bad, h, "one ulp off")
    bad_h = h.clone()
    bad_h.view(torch.int16)[36, 775] += 1
    with pytest.raises(AssertionError):
        t.check_ln_forward(c, mean, rstd, y, bad_h, "h one ulp off")
    # inside the band the other neighbour is accepted, two ulps away never
    ka = int(amb[20].nonzero()[0])
    lo, hi, near, _ = classify(c["y"], band=c["band"])
    other = y.clone()
    other[20, ka] = (lo if float(near[20, ka]) == float(hi[20, ka]) else hi)[20, ka]
    t.check_ln_forward(c, mean, rstd, other, h, "the other neighbour inside the band")


def test_check_banded_where_the_band_exceeds_the_spacing():
    """3.4e-4 has a bf16 spacing of 2^-19 = 1.9e-6: a band of 1e-5 spans eleven values, all accepted,
    and nothing beyond them; at 1.0 (spacing 2^-7) the same band reaches no midpoint: bit-exact."""
    v = torch.tensor([[3.4e-4, 1.0]], dtype=F64)
    band = torch.full_like(v, 1e-5)
    for k in (-0.9, 0.0, 0.9):
        t.check_banded(as_bf16(rne(v + k * band * torch.tensor([[1.0, 0.0]], dtype=F64))), v, band, "inside")
    for k in (-1.3, 1.3):
        with pytest.raises(AssertionError):
            t.check_banded(as_bf16(rne(v + k * band * torch.tensor([[1.0, 0.0]], dtype=F64))), v, band, "outside")
    with pytest.raises(AssertionError):
        t.check_banded(torch.tensor([[3.4e-4, 1.0078125]]).to(BF16), v, band, "one ulp off at 1.0")


def test_layernorm_checker_rejects_a_one_pass_variance():
    """An offset row whose variance is E[v^2] - mean^2 in fp32: rstd leaves its counted bound (y's band,
    which has to admit the mean's own error K_MEAN U A, is too wide at this offset to show it)."""
    c = t.ln_case(t.ADV_N, 776, "plain", adv=True)
    good = as_kernel_outputs(c)
    t.check_ln_forward(c, *good, None, "two-pass")
    one = t.ln_reference(c["v32"].to(F64), c["w"], c["b"], one_pass_row=1)
    mean, rstd, y = as_kernel_outputs(one)
    rel = float((one["rstd"][1] - c["rstd"][1]).abs() / c["rstd"][1])
    print(f"[ln-gelu-embed] one-pass rstd of the offset row is off by {rel:.2e}, bound {float(c['rstd_bound'][1]):.2e}")
    assert rel > float(c["rstd_bound"][1])
    with pytest.raises(AssertionError):
        t.check_ln_forward(c, mean, rstd, good[2], None, "one-pass rstd")


def test_layernorm_backward_checkers_reject_one_ulp():
    i = t.ln_bwd_inputs(37, 776, False)
    v = i["x"]
    mu = v.mean(1)
    rs = 1.0 / torch.sqrt(((v - mu[:, None]) ** 2).mean(1) + t.EPS)
    ref = t.ln_bwd_reference(v, i["dy"], i["w"], mu, rs, i["dres"])
    dx = as_bf16(rne(ref["dx"]))
    t.check_banded(dx, ref["dx"], ref["band"], "dx")
    _, _, _, amb = classify(ref["dx"], band=ref["band"])
    k = int((~amb[3]).nonzero()[0])
    bad = dx.clone()
    bad.view(torch.int16)[3, k] += 1
    with pytest.raises(AssertionError):
        t.check_banded(bad, ref["dx"], ref["band"], "dx one ulp off")
    for name in ("dgamma", "dbeta", "drbias"):
        s, bound = ref[name]
        got = as_bf16(rne(s))
        t.check_colgrad(name, got, ref, "reference")
        assert float((bound / s.abs().clamp_min(1e-300)).median()) < 2.0 ** -9   # the interval is about one value wide
        far = got.clone()
        col = int(s.abs().argmax())
        far.view(torch.int16)[col] += 2
        with pytest.raises(AssertionError):
            t.check_colgrad(name, far, ref, "two ulps off")


def test_gelu_checkers_reject_a_shifted_bias_column():
    """Outputs computed with the bias vector shifted by one column are rejected per element and per
    column; so is a single element one ulp off."""
    c = t.gelu_case(77, 3072)
    r = t.gelu_refs(c)
    y, dx = as_bf16(rne(r["y"])), as_bf16(rne(r["dx"]))
    check_activation(y, r["y"], "y")
    check_activation(dx, r["dx"], "dx")
    t.check_db(as_bf16(rne(r["db"])), c, r, "db")
    shifted = t.gelu_refs(c, b=torch.roll(c["b"], 1))
    with pytest.raises(AssertionError):
        check_activation(as_bf16(rne(shifted["y"])), r["y"], "y with a shifted bias")
    with pytest.raises(AssertionError):
        check_activation(as_bf16(rne(shifted["dx"])), r["dx"], "dx with a shifted bias")
    with pytest.raises(AssertionError):
        t.check_db(as_bf16(rne(shifted["db"])), c, r, "db with a shifted bias")
    # one column only
    b1 = c["b"].clone()
    b1[1234] = c["b"][1233]
    one = t.gelu_refs(c, b=b1)
    with pytest.raises(AssertionError):
        check_activation(as_bf16(rne(one["y"])), r["y"], "y with one wrong bias column")
    _, _, _, amb = classify(r["y"])
    k = int((~amb[5]).nonzero()[7])
    bad = y.clone()
    bad.view(torch.int16)[5, k] += 1
    with pytest.raises(AssertionError):
        check_activation(bad, r["y"], "y one ulp off")


def test_sweep_checker_zones_and_rejections():
    x = t.sweep_patterns()
    b = t.gelu_bias(1024, 0)
    arg = t.gelu_arg(x, b)
    v = t.gelu_ref(arg)
    finite = torch.where(arg.abs() <= t.SWEEP_LIMIT, v, torch.zeros_like(v))
    got = rne(torch.where(finite.abs() >= t.BAND_MIN, finite, torch.zeros_like(v))).to(torch.float32).to(BF16)
    zones = t.sweep_check(got, v, arg, "rounded reference")
    assert sum(zones) == 65536 and min(zones) > 1000
    bad = got.clone()
    k = int(((arg > 16) & (arg < 2.0 ** 30)).flatten().nonzero()[0])
    bad.view(-1)[k] = float("inf")
    with pytest.raises(AssertionError):
        t.sweep_check(bad, v, arg, "a non-finite value inside 2^40")
    bad = got.clone()
    bad.view(torch.int16).view(-1)[k] += 2
    with pytest.raises(AssertionError):
        t.sweep_check(bad, v, arg, "two ulps off in the relative zone")
    _, _, _, amb = classify(torch.where(arg.abs() <= 8, v, torch.ones_like(v)))
    k = int(((arg.abs() <= 8) & (v.abs() > 1e-3) & ~amb).flatten().nonzero()[0])
    bad = got.clone()
    bad.view(torch.int16).view(-1)[k] += 1
    with pytest.raises(AssertionError):
        t.sweep_check(bad, v, arg, "one ulp off in the band zone")
