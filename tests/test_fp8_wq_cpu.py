"""The step's e4m3 weight arena (FlatParams.enable_wq) off the GPU: a no-op, and the table its grouped quantiser reads."""
import pytest
import torch

from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
from paddle_operator_amd.parallel.flat import ALIGN, WQ_CHUNK, wq_table
from paddle_operator_amd.train import GPT2Trainer, fp8_weights


def test_enable_wq_is_a_noop_and_the_tiny_trainer_steps_with_fp8_ln_on_cpu():
    cfg = GPT2Config.named("gpt2-tiny")
    cfg.fp8 = "ln"
    tr = GPT2Trainer(cfg, 2, 32, "cpu", dtype=torch.float32, lr=6e-4)
    idx, tgt = tr.batch()
    losses = [float(tr.step(idx, tgt).detach()) for _ in range(2)]  # the same batch twice: the step must help
    assert losses[1] < losses[0]
    with tr.flat.wt_scope():
        assert tr.flat.wq is None and not tr.flat.wq_live and not hasattr(tr.model.blocks[0].qkv.weight, "_pdo_wq")


@pytest.mark.parametrize("name,fp8,melems", [("gpt2-smoke", "qkv", None), ("gpt2-smoke", "lnmx", None),
                                             ("gpt2-medium", "ln", 168), ("gpt2-medium", "lnmx", 264)])
def test_table_is_aligned_sorted_and_disjoint(monkeypatch, name, fp8, melems):
    monkeypatch.setattr(GPT2, "reset_parameters", lambda self: None)
    with torch.device("meta"):  # shapes only: nothing is allocated or drawn
        ws = fp8_weights(GPT2(GPT2Config.named(name)), fp8)
    segs = [(3 * i * ALIGN + sum(v.numel() for v in ws[:i]), w.numel()) for i, w in enumerate(ws)]  # ALIGN-aligned, gaps
    rows, chunks, nbytes = wq_table(segs)
    want_chunk = end = 0
    for (chunk, src, dst, n), seg in zip(rows, segs):
        assert (src, n) == seg and chunk == want_chunk and dst >= end
        assert src % 8 == 0 and n % 8 == 0 and dst % 16 == 0
        want_chunk, end = chunk + -(-n // WQ_CHUNK), dst + n
    assert chunks == want_chunk and end <= nbytes < end + 16
    assert not melems or sum(n for _, n in segs) == melems << 20
