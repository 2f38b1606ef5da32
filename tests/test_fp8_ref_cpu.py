"""ops.ref_quant_e4m3: the scale rule s = 2^e from the bits of amax, and the e4m3 round trip (CPU)."""
import pytest
import torch

from paddle_operator_amd import ops


def _next_up(v: float) -> float:
    t = torch.tensor([v], dtype=torch.float32)
    return float((t.view(torch.int32) + 1).view(torch.float32))


@pytest.mark.parametrize("a", [-20, -1, 0, 3, 17])
@pytest.mark.parametrize("m", ["1.0", "1.75", "above 1.75"])
def test_scale_puts_amax_in_the_top_binade(a, m):
    amax = {"1.0": 1.0, "1.75": 1.75, "above 1.75": _next_up(1.75)}[m] * 2.0 ** a
    x = torch.tensor([0.0, -amax, amax / 3], dtype=torch.float32)  # fp32 input: the boundary's neighbour is no bf16
    q, d = ops.ref_quant_e4m3(x)
    d = float(d)
    s = 1.0 / d
    assert d * s == 1.0
    assert 224.0 < amax * s <= 448.0
    assert s == 2.0 ** ((8 if m != "above 1.75" else 7) - a)
    assert q.dtype == torch.uint8 and q.shape == x.shape


def test_zeros_give_unit_scale():
    q, d = ops.ref_quant_e4m3(torch.zeros(4, 8, dtype=torch.bfloat16))
    assert float(d) == 1.0 and not q.any()


@pytest.mark.parametrize("p", [-9, 0, 6])
def test_round_trip_of_e4m3_values(p):
    # every finite e4m3 value (both signs) times 2^p is a bf16 and must come back unchanged
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).float()
    x = (vals[torch.isfinite(vals)] * 2.0 ** p).to(torch.bfloat16)
    q, d = ops.ref_quant_e4m3(x)
    assert torch.equal(q.view(torch.float8_e4m3fn).float() * d, x.float())
