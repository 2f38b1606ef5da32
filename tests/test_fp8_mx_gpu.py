"""GPT2Config.fp8 = "lnmx": fc1's GELU epilogue on gemm_nt_f8 writing MXFP8 rows (gemm_nt_f8_gelu(mx=True)), the scaled
MFMA GEMM that reads them (gemm_nt_mx8) with its three epilogues, and the routes through ops.mlp /
ops.mlp_add_layer_norm.  References are float64 or the plain-torch rule (ops.ref_quant_mx8_rows).

Measured on an MI355X (profiles/fp8_mx.md): Gaussian MXFP8 rows → GEMM with bias and residual worst |err| / bound =
0.952; gpt2-smoke |loss_lnmx − loss_fp32| / |loss_bf16 − loss_fp32| = 3.40 without residual dropout (losses 8.345421 /
8.345388 / 8.345398; "ln" 8.345423) and 47.0 with resid_pdrop = 0.1 (8.342998 / 8.343401 / 8.343410; "ln" 8.343554:
the bf16 error in the denominator is 9e-6), so the asserted multiples are 6.8 and 94.0.
"""
import functools

import pytest
import torch

from paddle_operator_amd import _native, ops

pytestmark = pytest.mark.gpu
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


@pytest.fixture(scope="module")
def m(cuda):
    return _native.require_hip()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("shape", [(256, 128, 256), (256, 256, 256), (512, 384, 512)], ids=str)
def test_fc1_epilogue_writes_the_reference_rows(m, cuda, shape):
    M, N, K = shape
    g = _gen(M + N + K)
    x = torch.randn(M, K, generator=g) * 2.0 ** (torch.arange(M) % 4).float().view(-1, 1)
    qa, da = (t.to(cuda) for t in ops.ref_quant_e4m3_rows(x.to(BF)))
    # W1's rows (= output columns) scaled per 32-column block over 2^−8 .. 2^5; block 1: zero rows under a large
    # negative bias, so gelu = (−)0 there and the block's byte is 127
    blk = torch.arange(N) // 32
    w1 = torch.randn(N, K, generator=g) * 0.05 * 2.0 ** ((5 * blk) % 14 - 8).float().view(-1, 1)
    b1 = 0.1 * torch.randn(N, generator=g)
    w1[32:64], b1[32:64] = 0.0, -30.0
    qb, db = m.quant_e4m3(w1.to(BF).to(cuda))
    b1 = b1.to(BF).to(cuda)
    g0, y0 = m.gemm_nt_f8_gelu(qa, da, qb, db, b1)
    g1, y1, q, s = m.gemm_nt_f8_gelu(qa, da, qb, db, b1, mx=True)
    assert torch.equal(g1, g0) and torch.equal(y1, y0)
    q_ref, s_ref = ops.ref_quant_mx8_rows(y1)
    assert torch.equal(s, s_ref), f"{int((s != s_ref).sum())} scale bytes differ"
    assert torch.equal(q, q_ref), f"{int((q != q_ref).sum())} bytes differ"
    assert s.unique().numel() >= 6 and (s[:, 1] == 127).all() and ((q & 0x7F) != 0).float().mean() > 0.5


@functools.lru_cache(maxsize=2)
def _int_case(cuda, M, N, K):
    """Operands e4m3 holds exactly, scale bytes distinct across a fragment's rows and a k-tile's blocks, and the
    float64 product (with db = 2^5); every partial sum is a multiple of 2⁻³ below 2²¹: exact in fp32."""
    g = _gen(M + 3 * N + 7 * K)
    a, b = (torch.randint(-3, 4, (r, K), generator=g).to(cuda) for r in (M, N))
    s = (127 + (5 * torch.arange(M).view(-1, 1) + 3 * torch.arange(K // 32).view(1, -1)) % 7 - 3).to(torch.uint8).to(cuda)
    bias, res = torch.randint(-8, 9, (N,), generator=g).to(cuda), torch.randint(-64, 65, (M, N), generator=g).to(cuda)
    ad = a.double() * torch.ldexp(torch.ones((), dtype=torch.float64, device=cuda), s.int() - 127).repeat_interleave(32, 1)
    prod = (ad @ b.double().t()) * 32.0
    db = torch.tensor([32.0], device=cuda)
    return a.float().to(F8).view(torch.uint8), s, b.float().to(F8).view(torch.uint8), db, bias, res, prod


@pytest.mark.parametrize("epi", ["plain", "bias", "bias+res"])
@pytest.mark.parametrize("shape", [(256, 256, 256), (256, 128, 512), (512, 384, 768), (256, 256, 1024), (4352, 4096, 512)],
                         ids=str)
def test_mx8_gemm_exact_on_integers(m, cuda, shape, epi):
    qa, s, qb, db, bias, res, prod = _int_case(cuda, *shape)
    kw = {"plain": {}, "bias": dict(bias=bias.to(BF)), "bias+res": dict(bias=bias.to(BF), res=res.to(BF))}[epi]
    c = m.gemm_nt_mx8(qa, s, qb, db, **kw)
    ref = prod + (bias.double() if epi != "plain" else 0.0) + (res.double() if epi == "bias+res" else 0.0)
    bad = c != ref.float().to(BF)
    assert not bad.any(), f"{int(bad.sum())} of {c.numel()} differ, first at {bad.nonzero()[0].tolist()}"
    if shape == (256, 256, 256) and epi == "plain":  # the case can tell: two scale columns swapped change the result
        assert not torch.equal(c, m.gemm_nt_mx8(qa, s[:, [1, 0] + list(range(2, s.shape[1]))].contiguous(), qb, db))


def test_mx8_gemm_within_fp32_accumulation_bound(m, cuda):
    """½ bf16 ulp of the float64 value + (K + 2)·2⁻²⁴·Σ|terms|: fp32 sums of K products, the bias and the residual.
    Worst |err| / bound measured on an MI355X: 0.952 (profiles/fp8_mx.md)."""
    M, N, K = 512, 384, 1024
    g = _gen(11)
    y = (torch.randn(M, K, generator=g) * 2.0 ** torch.randint(-9, 10, (M, K // 32), generator=g).repeat_interleave(32, 1)).to(BF)
    q, s = (t.to(cuda) for t in ops.ref_quant_mx8_rows(y))
    w, bias, res = ((torch.randn(*sh, generator=g) * sc).to(BF).to(cuda) for sh, sc in (((N, K), 0.02), ((N,), 0.1), ((M, N), 1.0)))
    qw, dw = m.quant_e4m3(w)
    c = m.gemm_nt_mx8(q, s, qw, dw, bias, res).double()
    a = q.view(F8).double() * torch.ldexp(torch.ones((), dtype=torch.float64, device=cuda), s.int() - 127).repeat_interleave(32, 1)
    b = qw.view(F8).double() * dw.double()
    ref = a @ b.t() + bias.double() + res.double()
    half_ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref).exponent - 9)  # |ref| ∈ [2^(e−1), 2^e): ulp 2^(e−8)
    mag = a.abs() @ b.abs().t() + bias.double().abs() + res.double().abs()
    ratio = ((c - ref).abs() / (half_ulp + (K + 2) * 2.0 ** -24 * mag)).max().item()
    print(f"worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def _route_case(cuda, C, B=2, S=256, seed=9):
    g = _gen(seed)
    mk = lambda *sh, e=-6: (torch.randn(*sh, generator=g) * 2.0 ** e).to(BF).to(cuda)  # noqa: E731
    h = mk(B, S, C, e=0)
    f8 = tuple(t.to(cuda) for t in ops.ref_quant_e4m3_rows(h))
    p = dict(w1=mk(4 * C, C), b1=mk(4 * C, e=-3), w2=mk(C, 4 * C), b2=mk(C, e=-3), res=mk(B, S, C, e=0),
             ln_w=1 + mk(C, e=-3), ln_b=mk(C, e=-3))
    return h, f8, p, mk(B, S, C, e=-4)


def _grads(fn, dy, *ts):
    ts = [t.detach().clone().requires_grad_() for t in ts]
    y = fn(*ts)
    (y[0] if isinstance(y, tuple) else y).backward(dy)  # the stream output: no LayerNorm of a different input behind it
    return [t.grad for t in ts]


@pytest.mark.parametrize("resid_pdrop", [0.0, 0.1])
def test_routes_are_the_two_kernels(m, cuda, resid_pdrop):
    h, f8, p, dy = _route_case(cuda, 256)
    q, s = m.gemm_nt_f8_gelu(*f8, *m.quant_e4m3(p["w1"]), p["b1"], mx=True)[2:]
    qw2 = m.quant_e4m3(p["w2"])
    plain = m.gemm_nt_mx8(q, s, *qw2).view(2, 256, 256)
    mlp_args = (h, p["w1"], p["b1"], p["w2"])
    y = ops.mlp(*mlp_args, f8=f8, mx=True)
    assert torch.equal(y, plain) and not torch.equal(y, ops.mlp(*mlp_args, f8=f8))
    drop = ops.dropout_spec(resid_pdrop, 77, 3, 5) if resid_pdrop else None
    args = mlp_args + (p["b2"], p["res"], p["ln_w"], p["ln_b"])
    hs, hn = ops.mlp_add_layer_norm(*args, drop=drop, f8=f8, mx=True)
    if drop is None:  # fc2's bias + residual epilogue
        assert torch.equal(hs, m.gemm_nt_mx8(q, s, *qw2, p["b2"], p["res"].view(-1, 256)).view(2, 256, 256))
    else:  # fc2's plain epilogue, bias and dropout in the add + LayerNorm pass
        want = ops.add_layer_norm(p["res"], plain, p["ln_w"], p["ln_b"], rbias=p["b2"], drop=drop)
        assert torch.equal(hs, want[0]) and torch.equal(hn, want[1])
    assert not torch.equal(hs, ops.mlp_add_layer_norm(*args, drop=drop, f8=f8)[0])
    # the saved tensors are the bf16 ones either way: the gradients are the "ln" route's bit for bit
    for fn, ts in ((ops.mlp, mlp_args), (functools.partial(ops.mlp_add_layer_norm, drop=drop), args)):
        for got, want in zip(_grads(functools.partial(fn, f8=f8, mx=True), dy, *ts), _grads(functools.partial(fn, f8=f8), dy, *ts)):
            assert (got is None and want is None) or torch.equal(got, want)


def test_routes_fall_back_outside_the_contract(cuda):
    h, f8, p, _ = _route_case(cuda, 320)  # K = 320 is no multiple of 256
    args = (h, p["w1"], p["b1"], p["w2"], p["b2"], p["res"], p["ln_w"], p["ln_b"])
    assert torch.equal(ops.mlp(*args[:4], f8=f8, mx=True), ops.mlp(*args[:4], f8=f8))
    assert torch.equal(ops.mlp_add_layer_norm(*args, f8=f8, mx=True)[0], ops.mlp_add_layer_norm(*args, f8=f8)[0])


LNMX_LOSS_ERR_FACTOR = {0.0: 6.8, 0.1: 94.0}  # × the bf16 path's own loss error; twice the measured ratios (profiles/fp8_mx.md)


@pytest.mark.parametrize("resid_pdrop", [0.0, 0.1])
def test_gpt2_smoke_step_with_fp8_lnmx(cuda, monkeypatch, resid_pdrop):
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    cfg = GPT2Config.named("gpt2-smoke")
    cfg.resid_pdrop = resid_pdrop
    with torch.device(cuda):
        ref = GPT2(cfg)  # fp32, same seed → same weights before the bf16 rounding
        model = GPT2(cfg).bfloat16()
    g = _gen(3)
    idx, tgt = (torch.randint(0, cfg.vocab_size, (4, 512), generator=g).to(cuda) for _ in range(2))
    with torch.no_grad():
        for p, q in zip(ref.parameters(), model.parameters()):
            p.copy_(q)
        monkeypatch.setenv("PDO_OPS", "torch")
        loss_ref = float(ref(idx, tgt))
        monkeypatch.setenv("PDO_OPS", "hip")
        loss_bf16 = float(model(idx, tgt))
        cfg.fp8 = "ln"
        loss_ln = float(model(idx, tgt))
    cfg.fp8 = "lnmx"
    loss = model(idx, tgt)
    loss.backward()
    loss_mx = float(loss.detach())
    e8, e16 = abs(loss_mx - loss_ref), abs(loss_bf16 - loss_ref)
    print(f"resid_pdrop {resid_pdrop}: fp32 {loss_ref:.6f} bf16 {loss_bf16:.6f} ln {loss_ln:.6f} lnmx {loss_mx:.6f}: ratio {e8 / max(e16, 1e-30):.3f}")
    assert loss_mx == loss_mx and loss_mx not in (loss_bf16, loss_ln)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert e8 <= LNMX_LOSS_ERR_FACTOR[resid_pdrop] * e16
