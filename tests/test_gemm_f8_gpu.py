"""The e4m3 quantiser and GEMM (csrc/hip/quant_f8.hip, gemm_nt_f8.hip) and their routes: ops.linear_fp8,
ops.qkv_attention(fp8=True), GPT2Config.fp8 = "qkv".

(a) quantiser bytes and scale == ops.ref_quant_e4m3, bit for bit; (b) the GEMM on small-integer operands ==
bf16(float64 product + bias), bit for bit (every partial sum is an integer < 2^24: exact in any order); (c) on
quantised Gaussian data within half a bf16 ulp + the fp32 accumulation bound of the float64 product; (d) autograd
and routing, bit for bit against the pieces; (e) one gpt2-smoke step against the fp32 model.

Measured on an MI355X: (c) worst |err| / bound = 0.912; (e) |loss_fp8 − loss_fp32| / |loss_bf16 − loss_fp32| =
3.40 (losses 8.345356 / 8.345388 / 8.345398), so the asserted multiple is 6.8 (profiles/fp8_qkv.md).
"""
import pytest
import torch

from paddle_operator_amd import _native, ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def m(cuda):
    return _native.require_hip()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- (a) quantiser
def _quant_input(kind):
    g = _gen(1)
    if kind == "contiguous":
        return torch.randn(256, 512, generator=g).to(BF)
    if kind == "strided":
        return torch.randn(64, 640, generator=g).to(BF)  # the test takes [:, :512]: ld 640 > 512 columns
    if kind.startswith("odd"):  # 20011 = 9 blocks' spans + 1579: a short last block and a 3-element tail
        x = (torch.randn(20011, generator=g) * 0.5).clamp(-3, 3).to(BF)
        x[{"odd-first": 0, "odd-last": 20010, "odd-mid": 10007}[kind]] = -7.0
        return x
    p = torch.arange(-6, 8).float().view(-1, 1)
    if kind == "ties":  # amax 448 → s = 1; (1 + odd/16)·2^p and (j + ½)·2^−9 sit midway between two e4m3 values
        t = ((1 + (2 * torch.arange(8).float() + 1) / 16) * 2.0 ** p).flatten()
        t = torch.cat([t, (torch.arange(8).float() + 0.5) * 2.0 ** -9])
        return torch.cat([t, -t, torch.tensor([448.0])]).to(BF)
    assert kind == "tiny"  # below e4m3's smallest normal 2^−6 at s = 1: subnormals and zeros
    return torch.cat([torch.randn(4093, generator=g) * 2.0 ** -8, torch.tensor([448.0])]).to(BF)


@pytest.mark.parametrize("kind", ["contiguous", "strided", "odd-first", "odd-last", "odd-mid", "ties", "tiny"])
def test_quantiser_matches_reference(m, cuda, kind):
    x = _quant_input(kind)
    xd = x.to(cuda)
    if kind == "strided":
        x, xd = x[:, :512], xd[:, :512]
    q, d = m.quant_e4m3(xd)
    q_ref, d_ref = ops.ref_quant_e4m3(x)
    assert torch.equal(d.cpu(), d_ref) and q.shape == x.shape
    assert torch.equal(q.cpu(), q_ref), f"{int((q.cpu() != q_ref).sum())} bytes differ"


# ---------------------------------------------------------------- (b) exact GEMM
def _int_case(cuda, M, N, K, lda_pad=0):
    g = _gen(M + 3 * N + 7 * K)
    a = torch.randint(-3, 4, (M, K + lda_pad), generator=g).float()
    b = torch.randint(-3, 4, (N, K), generator=g).float()
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    qa, qb = a.to(F8).view(torch.uint8).to(cuda), b.to(F8).view(torch.uint8).to(cuda)
    prod = a[:, :K].to(cuda).double() @ b.to(cuda).double().t()
    return qa[:, :K], qb, bias.to(cuda), prod


SHAPES = [(256, 256, 256), (256, 256, 512), (256, 128, 512), (512, 384, 768), (256, 256, 1024), (4352, 4096, 512)]


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("case", SHAPES + ["lda>K", "scales"], ids=str)
def test_gemm_exact_on_integers(m, cuda, case, with_bias):
    M, N, K = case if isinstance(case, tuple) else (512, 384, 768)
    qa, qb, bias, prod = _int_case(cuda, M, N, K, lda_pad=256 if case == "lda>K" else 0)
    da, db = (2.0 ** -3, 2.0 ** 5) if case == "scales" else (1.0, 1.0)
    one = lambda v: torch.tensor([v], dtype=torch.float32, device=cuda)  # noqa: E731
    c = m.gemm_nt_f8(qa, one(da), qb, one(db), bias.to(BF) if with_bias else None)
    ref = (prod * (da * db) + (bias.double() if with_bias else 0.0)).float().to(BF)
    bad = c != ref
    assert not bad.any(), f"{int(bad.sum())} of {c.numel()} differ, first at {bad.nonzero()[0].tolist()}"


# ---------------------------------------------------------------- (c) Gaussian data vs float64
def test_gemm_gaussian_within_fp32_accumulation_bound(m, cuda):
    M, N, K = 512, 384, 1024
    g = _gen(5)
    x, w = torch.randn(M, K, generator=g).to(BF), (torch.randn(N, K, generator=g) * 0.02).to(BF)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF)
    (qx, dx), (qw, dw) = m.quant_e4m3(x.to(cuda)), m.quant_e4m3(w.to(cuda))
    c = m.gemm_nt_f8(qx, dx, qw, dw, bias.to(cuda)).cpu().double()
    a = qx.cpu().view(F8).double() * dx.cpu().double()
    b = qw.cpu().view(F8).double() * dw.cpu().double()
    ref = a @ b.t() + bias.double()
    half_ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref).exponent - 9)  # |ref| ∈ [2^(e−1), 2^e): ulp 2^(e−8)
    bound = half_ulp + K * 2.0 ** -24 * (a.abs() @ b.abs().t())
    ratio = ((c - ref).abs() / bound).max().item()
    print(f"worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ---------------------------------------------------------------- (d) autograd and routing
def _params(cuda, B, S, C, N, seed=9):
    g = _gen(seed)
    mk = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(BF).to(cuda)  # noqa: E731
    return mk(B, S, C), mk(N, C, std=0.02), mk(N, std=0.1), mk(B, S, N, std=0.05)


def _grads(fn, x, w, b, dy):
    x, w, b = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y = fn(x, w, b)
    y.backward(dy)
    return y.detach(), x.grad, w.grad, b.grad


def test_linear_fp8_forward_and_backward(m, cuda):
    x, w, b, dy = _params(cuda, 2, 256, 256, 768)
    y, dx, dw, db = _grads(ops.linear_fp8, x, w, b, dy)
    (qx, sx), (qw, sw) = m.quant_e4m3(x.view(-1, 256)), m.quant_e4m3(w)
    assert torch.equal(y, m.gemm_nt_f8(qx, sx, qw, sw, b).view(2, 256, 768))
    assert not torch.equal(y, ops.linear(x, w, b))  # the e4m3 product, not the bf16 one
    for got, want in zip((dx, dw, db), _grads(ops.linear, x, w, b, dy)[1:]):
        assert torch.equal(got, want)


def test_linear_fp8_falls_back_outside_the_contract(cuda):
    x, w, b, _ = _params(cuda, 2, 128, 320, 768)
    assert torch.equal(ops.linear_fp8(x, w, b), ops.linear(x, w, b))


@pytest.mark.parametrize("fp8", [True, False])
def test_qkv_attention_route(cuda, fp8):
    h, w, b, _ = _params(cuda, 2, 256, 256, 768)
    o = ops.qkv_attention(h, w, b, 4, fp8=fp8)
    assert torch.equal(o, ops.attention((ops.linear_fp8 if fp8 else ops.linear)(h, w, b), 4))
    assert torch.equal(o, ops.qkv_attention(h, w, b, 4)) != fp8


# ---------------------------------------------------------------- (e) model
FP8_LOSS_ERR_FACTOR = 6.8  # × the bf16 path's own loss error; twice the measured ratio (profiles/fp8_qkv.md)


def test_gpt2_smoke_step_with_fp8_qkv(cuda, monkeypatch):
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    cfg = GPT2Config.named("gpt2-smoke")
    with torch.device(cuda):
        ref = GPT2(cfg)  # fp32, same seed → same weights before the bf16 rounding
        model = GPT2(cfg).bfloat16()
    g = _gen(3)
    idx = torch.randint(0, cfg.vocab_size, (4, 512), generator=g).to(cuda)
    tgt = torch.randint(0, cfg.vocab_size, (4, 512), generator=g).to(cuda)
    with torch.no_grad():
        for p, q in zip(ref.parameters(), model.parameters()):
            p.copy_(q)
    with torch.no_grad():
        monkeypatch.setenv("PDO_OPS", "torch")
        loss_ref = float(ref(idx, tgt))
        monkeypatch.setenv("PDO_OPS", "hip")
        loss_bf16 = float(model(idx, tgt))
    cfg.fp8 = "qkv"
    loss = model(idx, tgt)
    loss.backward()
    loss_fp8 = float(loss.detach())
    e8, e16 = abs(loss_fp8 - loss_ref), abs(loss_bf16 - loss_ref)
    print(f"loss fp32 {loss_ref:.6f} bf16 {loss_bf16:.6f} fp8 {loss_fp8:.6f}: ratio {e8 / max(e16, 1e-30):.3f}")
    assert loss_fp8 == loss_fp8 and loss_fp8 != loss_bf16
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert e8 <= FP8_LOSS_ERR_FACTOR * e16
