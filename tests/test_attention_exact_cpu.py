"""CPU checks of the builders, references and checkers of test_attention_exact_gpu.py: the float64
references against torch autograd, an emulation of the documented arithmetic of the three kernels
through every checker (with the running max at the true maximum, 7.9 below it, and on the defer-max
trajectory), the preconditions the GPU tests rely on, and sensitivity: each perturbed emulation of
the list below is rejected by the checker its test names.

The emulation also shows why the roundings are charged at u = 2^-8: at 2^-9 it reaches 1.2 - 1.6 of the
o and dQ bounds in rows of a few keys (module docstring of the GPU file)."""
import functools
import math

import pytest
import torch

import test_attention_exact_gpu as t
from test_gemm_nt_exact_gpu import as_bf16, rne

F64 = torch.float64
D = t.D
LOG2E_F32 = float(torch.tensor(t.LOG2E, dtype=torch.float32))
LN2_F32 = float(torch.tensor(t.LN2, dtype=torch.float32))
MID = (2, 256, 3)      # the shape most perturbations run at
BIG = (1, 512, 2)


def f32(x):
    return x.to(torch.float32).to(F64)


def bf(x):
    """fp32 value -> bf16 (RNE), as float64."""
    return rne(x)


def tril(S):
    return t.tril(S, "cpu")


# ---------------------------------------------------------------------------------------------
# the documented arithmetic, in float64 with the roundings at the documented places
# ---------------------------------------------------------------------------------------------
def emulate_forward(q, k, v, mode="defer", slack=0.0, mask=None, key_map=None, skip_rescale=False, lse_log2=False):
    """[B, H, S, D] float64 -> o bf16 [B, H, S, D], lse fp32 [B, H, S].  mode 'max': m = the row
    maximum - slack; 'defer': m set by tile 0 and moved when a 64-key tile exceeds it by more than 8.
    Perturbations: mask (another causal mask), key_map (K / V rows gathered through it),
    skip_rescale (m moves, l and acc are not multiplied by alpha), lse_log2 (no factor ln 2)."""
    S = q.shape[-2]
    qs = bf(f32(q * t.C2))
    if key_map is not None:
        k, v = k[..., key_map, :], v[..., key_map, :]
    tri = tril(S) if mask is None else mask
    s = (qs @ k.transpose(-1, -2)).masked_fill(~tri, -math.inf)
    if mode == "max":
        m = s.amax(-1) - slack
        P = bf(f32(torch.exp2(s - m[..., None])))
        l, acc = P.sum(-1), P @ v
    else:
        m = s[..., :64].amax(-1)
        l, acc = torch.zeros_like(m), torch.zeros_like(q)
        for c in range(0, S, 64):
            st = s[..., c:c + 64]
            if c:
                tm = st.amax(-1) - m
                d = torch.where(tm > 8.0, tm, torch.zeros_like(tm))
                m = m + d
                if not skip_rescale:
                    l, acc = l * torch.exp2(-d), acc * torch.exp2(-d)[..., None]
            P = bf(f32(torch.exp2(st - m[..., None])))
            l, acc = l + P.sum(-1), acc + P @ v[..., c:c + 64, :]
    lse = m + torch.log2(l)
    return as_bf16(rne(acc / l[..., None])), (lse if lse_log2 else f32(lse * LN2_F32)).to(torch.float32)


def emulate_backward(q, k, v, do, o, lse, dk_scale=True, dv_scale=False, neighbour_delta=False, query_map=None):
    """The dQ kernel, then dK / dV.  o bf16, lse fp32 as the forward gave them.  Perturbations: dK
    without scale, dV with scale, delta of the neighbouring row, query_map (the dK / dV kernel's Q,
    dO, lq and delta rows gathered through it: a stale ring slot)."""
    S = q.shape[-2]
    tri = tril(S)
    o, lse = o.double(), lse.double()
    lq = f32(lse * LOG2E_F32)
    delta = f32((do * o).sum(-1))
    if neighbour_delta:
        delta = torch.roll(delta, -1, -1)
    # dQ: P from the fma of the unrounded score, dS rounded once
    P = f32(torch.exp2(f32((q @ k.transpose(-1, -2)) * t.C2 - lq[..., None]))) * tri
    dS = bf(f32(P * (f32(do @ v.transpose(-1, -2)) - delta[..., None])))
    dq = rne(t.SCALE * (dS @ k))
    # dK / dV: the key prescaled, the chains start at -lq and -delta
    ks = bf(f32(k * t.C2))
    qq, dd, ll, de = q, do, lq, delta
    if query_map is not None:
        qq, dd, ll, de = q[..., query_map, :], do[..., query_map, :], lq[..., query_map], delta[..., query_map]
    P2 = f32(torch.exp2(f32(qq @ ks.transpose(-1, -2) - ll[..., None]))) * tri
    dS2 = bf(f32(P2 * f32(dd @ v.transpose(-1, -2) - de[..., None])))
    dv = rne((t.SCALE if dv_scale else 1.0) * (bf(P2).transpose(-1, -2) @ dd))
    dk = rne((t.SCALE if dk_scale else 1.0) * (dS2.transpose(-1, -2) @ qq))
    return as_bf16(dq), as_bf16(dk), as_bf16(dv)


@functools.lru_cache(maxsize=None)
def b_reference(kind, B, S, H):
    q, k, v, _ = t.b_case(kind, B, S, H)
    return t.forward_reference(q, k, v)


ALL_B = [(kind,) + shape for kind in t.KINDS for shape in t.SHAPES]


def _id(case):
    return f"{case[0]}-B{case[1]}-S{case[2]}-H{case[3]}"


# ---------------------------------------------------------------------------------------------
# references against torch autograd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("randn", "sharp"))
def test_references_match_torch_autograd(kind):
    """forward_reference is the explicit float64 attention, and the R2 formula equals its autograd
    gradients when lse and o are the exact ones."""
    B, S, H = MID
    q, k, v, do = (x.clone().requires_grad_(True) for x in t.b_case(kind, B, S, H))
    s = (t.SCALE * (q @ k.transpose(-1, -2))).masked_fill(~tril(S), -math.inf)
    o = torch.softmax(s, -1) @ v
    o.backward(do.detach())
    ref = b_reference(kind, B, S, H)
    assert float((ref["o"] - o.detach()).abs().max()) < 1e-13
    assert float((ref["lse"] - torch.logsumexp(s.detach(), -1)).abs().max()) < 1e-13
    assert float((ref["w"].sum(-1) - 1.0).abs().max()) < 1e-13
    r2 = t.backward_reference(q.detach(), k.detach(), v.detach(), do.detach(), ref["o"], ref["lse"])
    for name, g in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert float((r2[name] - g).abs().max()) < 1e-11 * max(1.0, float(g.abs().max())), name


def test_layout_helpers_round_trip():
    B, S, H = MID
    q, k, v, do = t.b_case("randn", B, S, H)
    x = t.pack_qkv(q, k, v).view(B, S, 3, H, D)
    assert torch.equal(x[1, 5, 0, 2].double(), q[1, 2, 5]) and torch.equal(x[0, 7, 1, 1].double(), k[0, 1, 7])
    assert torch.equal(x[1, 9, 2, 0].double(), v[1, 0, 9])
    assert torch.equal(t.to_heads(t.to_rows(do), H).double(), do)
    dq, dk, dv = t.split_dqkv(x.reshape(B, S, 3 * H * D), H)
    assert torch.equal(dq.double(), q) and torch.equal(dk.double(), k) and torch.equal(dv.double(), v)


# ---------------------------------------------------------------------------------------------
# preconditions
# ---------------------------------------------------------------------------------------------
def test_reciprocals_keep_clear_of_rounding_midpoints():
    """1 / n, n <= 512, lies at least 2^-16.1 (relative) from a bf16 midpoint, and the counted fp32
    errors of the forward's o and of the backward's P~ stay below that distance for every n."""
    n = torch.arange(1, 513, dtype=F64)
    dist = t.recip_midpoint_distance(n)
    k = int(dist.argmin())
    print(f"[attn-exact] closest 1 / n to a midpoint: n = {k + 1}, {float(dist[k]):.3e}; largest counted error "
          f"{float(t.a1_p_error(n).max()):.3e} = 2^{math.log2(float(t.a1_p_error(n).max())):.1f}")
    assert k + 1 in (255, 510) and float(dist[k]) > 2.0 ** -16.1
    assert bool((t.a1_o_error(n) < dist).all()) and bool((t.a1_p_error(n) < dist).all())
    assert float((t.a1_p_error(n) / dist).max()) < 0.25


@pytest.mark.parametrize("case", ALL_B, ids=_id)
def test_sigma_is_inside_the_model(case):
    sigma = float(b_reference(*case)["sigma"].max())
    print(f"[attn-exact] {_id(case)}: largest sigma {sigma:.4f}")
    assert sigma <= t.SIGMA_MAX


def test_selector_mix_and_signatures():
    """The selector rows keep their mix (rescaling rows and rows without a match at every S; 361 and
    88 at S = 512); the index maps cover all 64 dims; a matching pair scores 46.25 in log2 units
    exactly; neighbouring heads carry different factors; head H - 1 is populated in the last key tile."""
    for B, S, H in t.SHAPES:
        j, i = t.selector_maps(S)
        assert set(j.tolist()) == set(range(64)) and (S < 256 or set(i.tolist()) == set(range(64)))
        _, resc, nomatch = t.selector_mix(S)
        assert resc > 0 and nomatch > 0, (S, resc, nomatch)
        if S == 512:
            assert (resc, nomatch) == t.SEL_MIX_512
        sig = t.head_sig(B, H).flatten()
        assert all(float(sig[a]) != float(sig[a + 1]) for a in range(B * H - 1))
        _, _, v = t.a1_inputs(B, S, H, S - 64)
        assert int((v[B - 1, H - 1, S - 64:] != 0).sum()) == 64
        q, k, v, _ = t.selector_case(B, S, H)
        assert float(v[B - 1, H - 1, S - 64:].abs().sum()) > 0 and float(k[B - 1, H - 1, S - 64:].abs().sum()) > 0
        assert int((t.a2_pattern(B, S, H)[B - 1, H - 1, S - 64:] != 0).sum()) > 8
    assert float(bf(f32(torch.tensor(16.0 * t.C2, dtype=F64))) * 16.0) == t.SEL_MATCH
    assert t.spike_key(512) % 64 not in (0, 63) and t.BIG_S * 3 * t.BIG_H * D * 2 >= 1 << 31


# ---------------------------------------------------------------------------------------------
# the emulation passes every checker
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H", t.SHAPES, ids=t.SHAPE_IDS)
def test_emulation_passes_a1(B, S, H):
    z = torch.zeros(B, H, S, D, dtype=F64)
    o0, lse0 = emulate_forward(z, z, z)
    for base in range(0, S, 64):
        o, lse = emulate_forward(*t.a1_inputs(B, S, H, base))
        t.check_a1_forward(o, lse, B, S, H, base, f"emulated A1 window {base}")
        t.check_a1_backward(*emulate_backward(z, z, z, t.a1_do(B, S, H, base), o0, lse0), B, S, H, base,
                            f"emulated A1 query window {base}")


@pytest.mark.parametrize("B,S,H", t.SHAPES, ids=t.SHAPE_IDS)
def test_emulation_passes_a2(B, S, H):
    shares = []
    for kind in ("dq", "dk"):
        for base in range(0, S, 64):
            q, k, v, do = t.a2_inputs(B, S, H, base, kind)
            o, lse = emulate_forward(q, k, v)
            shares.append(t.check_a2(kind, base, o, lse, *emulate_backward(q, k, v, do, o, lse), B, S, H,
                                     f"emulated A2 {kind} window {base}"))
    print(f"[attn-exact] A2 {B}x{S}x{H}: largest midpoint share {max(shares):.3%}")


@pytest.mark.parametrize("B,S,H", t.SHAPES, ids=t.SHAPE_IDS)
def test_emulation_passes_a3(B, S, H):
    q, k, v, _ = t.selector_case(B, S, H)
    ref = b_reference("selector", B, S, H)
    o, lse = emulate_forward(q, k, v)
    share, rl = t.check_a3(o, lse, ref, v, B, S, H, "emulated A3")
    # the defer-max emulation and the float64 truth agree far inside the absolute term
    m = emulate_forward(q, k, v, mode="max")[0]
    assert float((o.double() - m.double()).abs().max()) < 1e-12
    print(f"[attn-exact] A3 {B}x{S}x{H}: midpoint share {share:.3%}, lse error / bound {rl:.3f}")


@pytest.mark.parametrize("case", ALL_B, ids=_id)
def test_emulation_passes_b(case):
    """Forward with m the true maximum, 7.9 below it and on the defer-max trajectory; backward from
    each forward's own outputs."""
    kind, B, S, H = case
    q, k, v, do = t.b_case(*case)
    ref = b_reference(*case)
    for name, kw in (("max", dict(mode="max")), ("max - 7.9", dict(mode="max", slack=7.9)), ("defer", {})):
        o, lse = emulate_forward(q, k, v, **kw)
        t.check_forward(ref, o, lse, f"emulated {_id(case)} m = {name}")
    r2 = t.backward_reference(q, k, v, do, o.double(), lse.double())
    t.check_backward(r2, *emulate_backward(q, k, v, do, o, lse), f"emulated {_id(case)}")


def test_emulated_bias_gradient_interval():
    """db = the rounded sum of the unrounded accumulators passes; a sum that misses one 128-row block
    of one head does not."""
    g = torch.Generator().manual_seed(5)
    B, S, H = MID
    acc = torch.randn(B, S, 3 * H * D, generator=g, dtype=F64)
    stored = as_bf16(rne(acc))
    db = as_bf16(rne(f32(acc.reshape(B * S, -1).sum(0))))
    assert t.check_db(db, stored, "emulated db") <= 1.0
    acc[1, 128:, :D] = 0.0
    with pytest.raises(AssertionError):
        t.check_db(as_bf16(rne(acc.reshape(B * S, -1).sum(0))), stored, "db without a block")


# ---------------------------------------------------------------------------------------------
# sensitivity: every perturbed emulation is rejected, by the checker named here
# ---------------------------------------------------------------------------------------------
def a1_forward_rejects(B, S, H, base, **kw):
    o, lse = emulate_forward(*t.a1_inputs(B, S, H, base), **kw)
    with pytest.raises(AssertionError):
        t.check_a1_forward(o, lse, B, S, H, base, "perturbed A1")
    return o, lse


def test_rejects_one_wrongly_unmasked_key():
    """Key q + 1 visible to row q = 200 alone: A1's bit check sees it (a non-zero above the diagonal
    and the row's 1 / (q + 2)); the randn bound does not have to (its figure is printed)."""
    B, S, H = MID
    mask = tril(S).clone()
    mask[200, 201] = True
    a1_forward_rejects(B, S, H, 192, mask=mask)
    q, k, v, _ = t.b_case("randn", B, S, H)
    o, _ = emulate_forward(q, k, v, mode="max", mask=mask)
    ref = b_reference("randn", B, S, H)
    print(f"[attn-exact] one unmasked key on randn: {t.worst(t.beyond_rounding(o, ref['o']), ref['Bo']):.2f} of Bo")


def test_rejects_a_skipped_32_key_block():
    """Keys 32 .. 63 missing for one wave's 32 rows: family B on randn (several times Bo)."""
    B, S, H = BIG
    mask = tril(S).clone()
    mask[480:512, 32:64] = False
    q, k, v, _ = t.b_case("randn", B, S, H)
    o, lse = emulate_forward(q, k, v, mask=mask)
    ref = b_reference("randn", B, S, H)
    print(f"[attn-exact] a skipped 32-key block: {t.worst(t.beyond_rounding(o, ref['o']), ref['Bo']):.2f} of Bo")
    with pytest.raises(AssertionError):
        t.check_forward(ref, o, lse, "a skipped block")


def test_rejects_stale_tiles():
    """A key tile read from the previous tile's buffer (A1 forward), and a dK / dV ring slot three
    tiles stale (A1 backward, dV)."""
    B, S, H = BIG
    key_map = torch.arange(S)
    key_map[128:192] = key_map[64:128]
    a1_forward_rejects(B, S, H, 128, key_map=key_map)
    z = torch.zeros(B, H, S, D, dtype=F64)
    o0, lse0 = emulate_forward(z, z, z)
    qmap = torch.arange(S)
    qmap[256:320] = qmap[64:128]
    with pytest.raises(AssertionError):
        t.check_a1_backward(*emulate_backward(z, z, z, t.a1_do(B, S, H, 256), o0, lse0, query_map=qmap), B, S, H, 256,
                            "a stale ring slot")


def test_rejects_swapped_column_halves():
    """The two 32-column halves of one row exchanged: A1 where the diagonal crosses the window (a
    row past the window holds one value in all 64 columns), A3 in any row."""
    B, S, H = MID
    swap = lambda row: torch.cat([row[32:], row[:32]])      # noqa: E731
    o, lse = emulate_forward(*t.a1_inputs(B, S, H, 64))
    o[1, 2, 100] = swap(o[1, 2, 100])
    with pytest.raises(AssertionError):
        t.check_a1_forward(o, lse, B, S, H, 64, "swapped halves")
    q, k, v, _ = t.selector_case(B, S, H)
    o, lse = emulate_forward(q, k, v)
    o[1, 2, 130] = swap(o[1, 2, 130])
    with pytest.raises(AssertionError):
        t.check_a3(o, lse, b_reference("selector", B, S, H), v, B, S, H, "swapped halves")


def test_rejects_a_zero_last_key_tile_of_the_last_head():
    """The last key tile of head H - 1 read as zeros (a buffer extent one tile short): A1 on its
    last window."""
    B, S, H = MID
    q, k, v = t.a1_inputs(B, S, H, S - 64)
    v = v.clone()
    v[B - 1, H - 1, S - 64:] = 0.0
    o, lse = emulate_forward(q, k, v)
    with pytest.raises(AssertionError):
        t.check_a1_forward(o, lse, B, S, H, S - 64, "a short extent")


def test_rejects_exchanged_heads():
    """Two heads' outputs exchanged: A1, through the heads' power-of-two factors."""
    B, S, H = BIG
    o, lse = emulate_forward(*t.a1_inputs(B, S, H, 0))
    with pytest.raises(AssertionError):
        t.check_a1_forward(o[:, [1, 0]], lse, B, S, H, 0, "exchanged heads")
    z = torch.zeros(B, H, S, D, dtype=F64)
    dq, dk, dv = emulate_backward(z, z, z, t.a1_do(B, S, H, 0), *emulate_forward(z, z, z))
    with pytest.raises(AssertionError):
        t.check_a1_backward(dq, dk, dv[:, [1, 0]], B, S, H, 0, "exchanged heads")


def test_rejects_a_skipped_rescale():
    """m moves by more than 8 and l and acc are not multiplied by alpha: A3 (o and lse)."""
    B, S, H = BIG
    q, k, v, _ = t.selector_case(B, S, H)
    o, lse = emulate_forward(q, k, v, skip_rescale=True)
    ref = b_reference("selector", B, S, H)
    with pytest.raises(AssertionError):
        t.check_a3(o, lse, ref, v, B, S, H, "a skipped rescale")
    good = emulate_forward(q, k, v)
    with pytest.raises(AssertionError):
        t.check_a3(good[0], lse, ref, v, B, S, H, "a skipped rescale, lse alone")
    with pytest.raises(AssertionError):
        t.check_forward(ref, o, good[1], "a skipped rescale, family B")


def test_rejects_lse_in_log2_units():
    """lse without the factor ln 2: A1's lse check."""
    B, S, H = MID
    o, lse = a1_forward_rejects(B, S, H, 0, lse_log2=True)
    t.check_bits(t.flat2(o), t.flat2(t.a1_o_expect(B, S, H, 0)), "o is untouched")


def a2_backward(B, S, H, base, kind, **kw):
    q, k, v, do = t.a2_inputs(B, S, H, base, kind)
    o, lse = emulate_forward(q, k, v)
    return (kind, base, o, lse) + emulate_backward(q, k, v, do, o, lse, **kw) + (B, S, H, "perturbed A2")


def test_rejects_dk_without_scale():
    """dK stored without the factor 1 / 8: A2's dK check."""
    with pytest.raises(AssertionError):
        t.check_a2(*a2_backward(*MID, 64, "dk", dk_scale=False))


def test_rejects_dv_with_scale():
    """dV stored with the factor 1 / 8: A1's dV check."""
    B, S, H = MID
    z = torch.zeros(B, H, S, D, dtype=F64)
    o0, lse0 = emulate_forward(z, z, z)
    with pytest.raises(AssertionError):
        t.check_a1_backward(*emulate_backward(z, z, z, t.a1_do(B, S, H, 64), o0, lse0, dv_scale=True), B, S, H, 64,
                            "dV with scale")


def test_rejects_the_neighbouring_rows_delta():
    """delta of row q + 1 used for row q: A2, dQ and dK."""
    for kind in ("dq", "dk"):
        with pytest.raises(AssertionError):
            t.check_a2(*a2_backward(*MID, 64, kind, neighbour_delta=True))
