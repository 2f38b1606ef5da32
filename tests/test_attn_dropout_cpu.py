"""Attention-probability dropout on the CPU: the host reference of the 4 × 4-patch
mask (``ops.core.philox_attn_keep_mask``, the mask the flash kernels draw, see
csrc/hip/philox.h), its statistics, and the model with ``attn_pdrop`` > 0 —
repeatable, distinct per step, off in eval, resumable from a checkpoint.

tests/test_attn_dropout_gpu.py recovers the kernels' masks bit for bit against
the same reference.
"""
import math

import numpy as np
import torch

from paddle_operator_amd import ops
from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
from paddle_operator_amd.ops.core import (ATTN_SITE0, _attn_patch_words, attn_dropout_spec, philox4x32_10,
                                          philox_attn_keep_mask, ref_attention)
from paddle_operator_amd.train import GPT2Trainer

SEED = 0x9E3779B97F4A7C15  # both key words non-zero


def _keep_by_definition(b, h, q, k, H, S, thr8, seed, site, step, bh0=0):
    """Element (q, k) straight from the definition: python ints, one Philox call."""
    P = S // 4
    g = ((bh0 + b * H + h) * P + q // 4) * P + k // 4
    w = philox4x32_10((g & 0xFFFFFFFF, g >> 32, site, step), (seed & 0xFFFFFFFF, seed >> 32))
    byte = (int(w[q % 4]) >> (8 * (k % 4))) & 0xFF
    return byte >= thr8


def test_mask_is_the_documented_function_of_philox():
    B, H, S, thr8, site, step = 2, 3, 256, 77, ATTN_SITE0 + 5, 11
    m = philox_attn_keep_mask(B, H, S, thr8, SEED, site, step)
    assert m.shape == (B, H, S, S) and m.dtype == torch.bool
    edges = [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255]  # patch and 32 / 64 / 128 boundaries
    for b, h in ((0, 0), (1, 2), (0, 1)):
        for q in edges:
            for k in edges:
                assert bool(m[b, h, q, k]) == _keep_by_definition(b, h, q, k, H, S, thr8, SEED, site, step), (b, h, q, k)


def test_patch_index_beyond_32_bits():
    """g ≥ 2^32: the counter's second word takes g's high half — through ``bh0`` (a slice of
    a large batch) and on the split itself."""
    H, S, thr8, site, step = 2, 8, 100, ATTN_SITE0, 3
    bh0 = 1 << 31  # P = 2: g = (bh·2 + q4)·2 + k4 ≥ 2^33
    m = philox_attn_keep_mask(1, H, S, thr8, SEED, site, step, bh0=bh0)
    for h in range(H):
        for q in range(S):
            for k in range(S):
                assert bool(m[0, h, q, k]) == _keep_by_definition(0, h, q, k, H, S, thr8, SEED, site, step, bh0), (h, q, k)
    g = np.array([(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (5 << 32) + 7], dtype=np.uint64)
    words = _attn_patch_words(g, SEED, site, step)
    for i, gi in enumerate(int(x) for x in g):
        want = philox4x32_10((gi & 0xFFFFFFFF, gi >> 32, site, step), (SEED & 0xFFFFFFFF, SEED >> 32))
        assert [int(w[i]) for w in words] == [int(w) for w in want]
    assert [int(w[0]) for w in words] != [int(w[1]) for w in words]


def test_mask_changes_with_seed_site_and_step():
    B, H, S, thr8 = 1, 2, 128, 128
    base = philox_attn_keep_mask(B, H, S, thr8, 1, ATTN_SITE0, 0)
    assert torch.equal(base, philox_attn_keep_mask(B, H, S, thr8, 1, ATTN_SITE0, 0))
    n = base.numel()
    for other in (philox_attn_keep_mask(B, H, S, thr8, 2, ATTN_SITE0, 0),
                  philox_attn_keep_mask(B, H, S, thr8, 1 + (1 << 32), ATTN_SITE0, 0),
                  philox_attn_keep_mask(B, H, S, thr8, 1, ATTN_SITE0 + 1, 0),
                  philox_attn_keep_mask(B, H, S, thr8, 1, ATTN_SITE0, 1)):
        # independent fair masks agree on half the elements: 5σ of n/2 ± √n/2
        agree = int((other == base).sum())
        assert abs(agree - n / 2) < 5 * math.sqrt(n) / 2, agree


def test_keep_fraction_over_the_causal_triangle():
    B, H, S, thr8 = 2, 2, 256, 26
    keep = philox_attn_keep_mask(B, H, S, thr8, 0xC0FFEE, ATTN_SITE0, 0)
    tri = torch.ones(S, S, dtype=torch.bool).tril()
    n = B * H * int(tri.sum())
    frac = float(keep[:, :, tri].double().mean())
    p = thr8 / 256.0
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(frac - 230 / 256) < 4 * sigma, (frac, 230 / 256, sigma)


def test_spec_quantisation_and_sites():
    assert attn_dropout_spec(0.0, 1, ATTN_SITE0, 0) is None and attn_dropout_spec(0.001, 1, ATTN_SITE0, 0) is None
    d = attn_dropout_spec(0.1, 5, ATTN_SITE0 + 3, 9)
    assert (d.thr, d.seed, d.site, d.step) == (26, 5, 0x10003, 9)
    assert d.scale == float(np.float32(256.0) / np.float32(230))
    assert attn_dropout_spec(0.75, 1, ATTN_SITE0, 0).scale == 4.0 and attn_dropout_spec(1.0, 1, ATTN_SITE0, 0).thr == 255
    # disjoint from the embedding / residual sites of any realistic depth
    assert ATTN_SITE0 > 2 + 2 * 1000


def test_attention_op_applies_the_host_mask():
    """ops.attention(drop=) on the CPU == the explicit softmax with the host mask; differentiable."""
    B, S, H, D = 2, 20, 2, 8
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * D, generator=g, requires_grad=True)
    d = attn_dropout_spec(0.3, SEED, ATTN_SITE0 + 1, 4)
    o = ops.attention(qkv, H, drop=d)
    q, k, v = qkv.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    keep = philox_attn_keep_mask(B, H, S, d.thr, d.seed, d.site, d.step)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(D)
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    want = (torch.softmax(s, -1) * keep * d.scale) @ v
    assert torch.allclose(o, want.transpose(1, 2).reshape(B, S, H * D), atol=1e-6)
    assert torch.equal(ref_attention(q, k, v), ops.attention(qkv, H).view(B, S, H, D).transpose(1, 2))
    assert torch.equal(ops.attention(qkv, H, drop=None), ops.attention(qkv, H))
    assert torch.equal(ops.qkv_attention(qkv[..., :16], torch.eye(48, 16), torch.zeros(48), H, drop=d),
                       ops.attention(qkv[..., :16] @ torch.eye(48, 16).t(), H, drop=d))
    o.sum().backward()
    assert qkv.grad is not None and bool(torch.isfinite(qkv.grad).all())


def _tiny(p=0.0, attn=0.0):
    cfg = GPT2Config.named("gpt2-tiny")
    cfg.embd_pdrop = cfg.resid_pdrop = p
    cfg.attn_pdrop = attn
    return cfg


def _batch(cfg, B=2, S=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, cfg.vocab_size, (B, S + 1), generator=g)
    return idx[:, :-1], idx[:, 1:]


def test_model_repeatable_distinct_and_eval():
    """attn_pdrop = 0.2 with drop_seed / drop_step set: two training forwards are bit-identical
    (the masks are a function of (seed, step, site, b, h, q, k), not of a framework RNG), another
    step differs, eval is the p = 0 model."""
    m0, m1 = GPT2(_tiny(0.0)), GPT2(_tiny(0.0, 0.2))
    m1.load_state_dict(m0.state_dict())
    m1.drop_seed, m1.drop_step = 99, 3
    x, y = _batch(m0.cfg)
    m1.train()
    la, lb = m1(x, y), m1(x, y)
    assert torch.equal(la, lb)
    assert not torch.equal(la, m0.train()(x, y))
    m1.drop_step = 4
    lc = m1(x, y)
    assert not torch.equal(lc, la)
    m1.drop_step = 3
    m1.drop_seed = 100
    assert not torch.equal(m1(x, y), la)
    assert torch.equal(m1.eval()(x, y), m0.eval()(x, y))
    m1.train()
    m1.drop_seed = 99
    ld = m1(x, y)
    assert torch.equal(ld, la)
    ld.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m1.parameters())


def test_resume_reproduces_the_next_step_with_attention_dropout():
    cfg = _tiny(0.1, 0.2)
    dev = torch.device("cpu")
    tr = GPT2Trainer(cfg, 2, 32, dev, dtype=torch.float32, dropout_seed=5)
    batches = [_batch(cfg, seed=s) for s in range(3)]
    for k in range(2):
        tr.step(*batches[k])
    st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in tr.state_dict().items()}
    st["opt"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st["opt"].items()}
    assert st["drop_step"] == 2
    want = float(tr.step(*batches[2]).detach())
    tr2 = GPT2Trainer(cfg, 2, 32, dev, dtype=torch.float32, dropout_seed=5)
    tr2.load_state_dict(st)
    assert float(tr2.step(*batches[2]).detach()) == want
    # the attention masks matter to that loss: without them the step differs
    tr3 = GPT2Trainer(_tiny(0.1, 0.0), 2, 32, dev, dtype=torch.float32, dropout_seed=5)
    tr3.load_state_dict(st)
    assert float(tr3.step(*batches[2]).detach()) != want
    tr4 = GPT2Trainer(cfg, 2, 32, dev, dtype=torch.float32, dropout_seed=6)
    tr4.load_state_dict(st)
    assert float(tr4.step(*batches[2]).detach()) != want
