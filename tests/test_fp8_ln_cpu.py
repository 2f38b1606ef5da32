"""GPT2Config.fp8 = "ln" off the GPU: the per-token e4m3 rule, the config values, the plain-torch model path."""
import pytest
import torch

from paddle_operator_amd import ops
from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config


def test_rows_reference_is_the_per_tensor_rule_per_row():
    g = torch.Generator().manual_seed(0)
    y = torch.randn(9, 64, generator=g) * 2.0 ** torch.arange(-4, 5).float().view(-1, 1)
    y[2] = 0.0  # amax 0 → e = 0, dscale 1
    y[3, 5], y[4, 7] = 1.75 * 2.0 ** 9, -1.7578125 * 2.0 ** 9  # the mantissa boundary (e = 8 − a) and one bf16 step past it
    y = y.to(torch.bfloat16)
    q, d = ops.ref_quant_e4m3_rows(y)
    assert q.shape == y.shape and q.dtype == torch.uint8 and d.shape == (9,) and d.dtype == torch.float32
    for r in range(9):
        qr, dr = ops.ref_quant_e4m3(y[r])
        assert torch.equal(q[r], qr) and d[r] == dr[0], r
    assert d[2] == 1.0 and d[3] == 2.0 and d[4] == 4.0


def test_config_values():
    assert GPT2Config(fp8="ln").fp8 == "ln"
    with pytest.raises(ValueError):
        GPT2Config(fp8="nonsense")


def test_tiny_model_reference_path():
    cfg = GPT2Config.named("gpt2-tiny")
    model = GPT2(cfg)
    g = torch.Generator().manual_seed(1)
    idx, tgt = (torch.randint(0, cfg.vocab_size, (2, 64), generator=g) for _ in range(2))
    with torch.no_grad():
        loss_off = float(model(idx, tgt))
    cfg.fp8 = "ln"
    loss = model(idx, tgt)
    loss.backward()
    assert torch.isfinite(loss) and float(loss) != loss_off
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
