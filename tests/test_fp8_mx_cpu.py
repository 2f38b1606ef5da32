"""The MXFP8 block rule and product in plain torch (ops.ref_quant_mx8_rows, ops.ref_linear_mx8_rows)."""
import pytest
import torch

from paddle_operator_amd import ops
from paddle_operator_amd.models.gpt2 import GPT2Config


def test_block_rule_on_hand_made_blocks():
    y = torch.zeros(2, 128)
    y[0, 0:32] = torch.linspace(-1.75, 1.0, 32)  # amax 1.75 = 1.75·2^0: m ≤ 1.75 → e = 8, 1.75·256 = 448
    y[0, 32] = 1.7578125                         # the next bf16 mantissa above 1.75 → e = 7, 225 → e4m3 224
    y[0, 96:128] = 3.5 * 2.0 ** -7               # 448·2^−14 → e = 14, exactly 448 after scaling
    y[1, 0] = 2.0 ** -126                        # e = 8 + 126 clamps to 126
    y[1, 64] = 2.0 ** 127                        # e = 8 − 127 = −119
    q, s = ops.ref_quant_mx8_rows(y.bfloat16())
    assert q.shape == (2, 128) and s.shape == (2, 4) and q.dtype == s.dtype == torch.uint8
    assert s[0].tolist() == [127 - 8, 127 - 7, 127, 127 - 14] and s[1].tolist() == [1, 127, 246, 127]
    f = q.view(torch.float8_e4m3fn).float()
    assert f[0, 0] == -448 and f[0, 31] == 256 and f[0, 32] == 224 and (f[0, 96:] == 448).all()
    assert not q[0, 64:96].any() and f[1, 0] == 1.0 and f[1, 64] == 256
    back = ops.ref_linear_mx8_rows(q, s, torch.eye(128).bfloat16(), dtype=torch.float32)  # W = I: dw = 2^−8, exact
    assert back[0, 0] == -1.75 and back[0, 96] == y[0, 96] and back[1, 0] == 2.0 ** -126 and back[1, 64] == 2.0 ** 127


def test_product_dequantises_blocks_and_rounds_once():
    g = torch.Generator().manual_seed(0)
    y = (torch.randn(5, 96, generator=g) * 2.0 ** torch.randint(-9, 10, (5, 3), generator=g).repeat_interleave(32, 1)).bfloat16()
    w, b, res = (torch.randn(*sh, generator=g).bfloat16() for sh in ((7, 96), (7,), (5, 7)))
    q, s = ops.ref_quant_mx8_rows(y)
    a = q.view(torch.float8_e4m3fn).double() * torch.ldexp(torch.ones(5, 3, dtype=torch.float64), s.int() - 127).repeat_interleave(32, 1)
    wq = ops.ref_quant_e4m3(w)
    wd = wq[0].view(torch.float8_e4m3fn).double() * wq[1].double()
    want = a @ wd.t() + b.double() + res.double()
    got = ops.ref_linear_mx8_rows(q, s, w, b, res)
    # one rounding of the fp32 sum: half a bf16 ulp of the float64 value (|want| ∈ [2^(e−1), 2^e): ulp 2^(e−8)) plus
    # the fp32 summation error of 96 + 2 terms, 98·2⁻²⁴ of the sum of their magnitudes
    half_ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want).exponent - 9)
    mag = a.abs() @ wd.abs().t() + b.double().abs() + res.double().abs()
    assert got.dtype == torch.bfloat16 and ((got.double() - want).abs() <= half_ulp + 98 * 2.0 ** -24 * mag).all()
    assert (a - y.double()).abs().max() <= (y.double().abs().reshape(5, 3, 32).amax(2) * 2.0 ** -4).max()  # e4m3: 3 mantissa bits


def test_config_does_not_offer_the_mode_without_kernels():
    with pytest.raises(ValueError):
        GPT2Config(vocab_size=128, n_positions=32, n_embd=32, n_layer=1, n_head=2, fp8="mx")
