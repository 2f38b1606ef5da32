"""Counter-based dropout on the CPU: the Philox host reference, the masks'
statistics and independence, train / eval / p = 0 behaviour of the model, resume
from a checkpoint, and the launcher flags.

The HIP kernels draw the same masks (csrc/hip/philox.h); tests/test_dropout_gpu.py
compares them with ``philox_keep_mask`` bit for bit.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
from paddle_operator_amd.ops.core import dropout_spec, dropout_thr, philox4x32_10, philox_keep_mask
from paddle_operator_amd.train import GPT2Trainer, derive_dropout_seed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# Random123 known-answer vectors of philox4x32-10 (counter; key → output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w) for w in philox4x32_10(ctr, key))
    assert got == want, [hex(g) for g in got]


def test_mask_is_the_documented_function_of_philox():
    """Element j of group g: word j >> 1 of philox((g_lo, g_hi, site, step); seed halves),
    low half for even j, high half for odd j, kept iff ≥ thr — including a group index
    past 2^32 through ``offset``."""
    seed, site, step, thr = 0x0123456789ABCDEF, 7, 11, 30000
    off = (1 << 32) - 2
    m = philox_keep_mask((4, 16), thr, seed, site, step, offset=off).reshape(-1, 8)
    for gi in range(8):
        g = off + gi
        w = [int(x) for x in philox4x32_10((g & 0xFFFFFFFF, g >> 32, site, step), (seed & 0xFFFFFFFF, seed >> 32))]
        for j in range(8):
            v = (w[j >> 1] >> 16) if j & 1 else (w[j >> 1] & 0xFFFF)
            assert bool(m[gi, j]) == (v >= thr), (gi, j)


def test_threshold_quantisation():
    assert dropout_thr(0.0) == 0 and dropout_thr(0.5) == 32768 and dropout_thr(0.1) == 6554
    assert dropout_thr(1.0) == 65535 and dropout_thr(-1.0) == 0
    assert dropout_spec(0.0, 1, 0, 0) is None and dropout_spec(1e-6, 1, 0, 0) is None  # quantises to thr 0
    d = dropout_spec(0.75, 5, 3, 9)
    assert (d.thr, d.scale, d.seed, d.site, d.step) == (49152, 4.0, 5, 3, 9)
    assert dropout_spec(0.1, 1, 0, 0).scale == float(np.float32(65536.0) / np.float32(65536 - 6554))


def test_keep_fraction():
    n = 1 << 20
    thr = dropout_thr(0.1)
    p = thr / 65536.0
    keep = philox_keep_mask((n // 1024, 1024), thr, 0xC0FFEE, 0, 0)
    frac = float(keep.double().mean())
    sigma = math.sqrt(p * (1 - p) / n)  # ≈ 2.9e-4
    assert abs(frac - (1 - p)) < 5 * sigma, (frac, 1 - p, sigma)


def test_mask_independence_and_offset():
    shape, thr = (64, 256), dropout_thr(0.5)
    base = philox_keep_mask(shape, thr, 1, 0, 0)
    assert torch.equal(base, philox_keep_mask(shape, thr, 1, 0, 0))
    n = base.numel()
    for other in (philox_keep_mask(shape, thr, 1, 1, 0), philox_keep_mask(shape, thr, 1, 0, 1),
                  philox_keep_mask(shape, thr, 2, 0, 0), philox_keep_mask(shape, thr, 1 << 32, 0, 0),
                  philox_keep_mask(shape, thr, derive_dropout_seed(1, 0), 0, 0),
                  philox_keep_mask(shape, thr, derive_dropout_seed(1, 1), 0, 0)):
        # independent fair masks agree on half the elements: 5σ of n/2 ± √n/2
        agree = int((other == base).sum())
        assert abs(agree - n / 2) < 5 * math.sqrt(n) / 2, agree
    a, b = derive_dropout_seed(1, 0), derive_dropout_seed(1, 1)
    assert a != b and a == derive_dropout_seed(1, 0) and 0 <= a < 1 << 64 and 0 <= b < 1 << 64
    k = 37  # groups
    tail = philox_keep_mask((64 * 256 // 8 - k, 8), thr, 1, 0, 0, offset=k)
    assert torch.equal(tail.reshape(-1), base.reshape(-1)[8 * k:])


def _tiny(p=0.0, attn=0.0):
    cfg = GPT2Config.named("gpt2-tiny")
    cfg.embd_pdrop = cfg.resid_pdrop = p
    cfg.attn_pdrop = attn
    return cfg


def _batch(cfg, B=2, S=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, cfg.vocab_size, (B, S + 1), generator=g)
    return idx[:, :-1], idx[:, 1:]


def test_train_eval_and_p0():
    m0, m1 = GPT2(_tiny(0.0)), GPT2(_tiny(0.1, 0.1))
    m1.load_state_dict(m0.state_dict())
    m1.drop_seed, m1.drop_step = 99, 3
    x, y = _batch(m0.cfg)
    l0 = m0(x, y)
    assert torch.equal(m1.eval()(x, y), m0.eval()(x, y))  # eval: dropout off, exactly the p = 0 model
    assert torch.equal(m0.train()(x, y), l0)
    m1.train()
    m1.cfg.attn_pdrop = 0.0  # the counter-based sites alone: repeatable
    la, lb = m1(x, y), m1(x, y)
    assert torch.equal(la, lb) and not torch.equal(la, l0)
    m1.drop_step = 4
    assert not torch.equal(m1(x, y), la)
    logits0, logits1 = m0(x), m1(x)
    assert logits0.shape == logits1.shape and not torch.equal(logits0, logits1)
    la.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m1.parameters())


def test_attention_dropout_cpu():
    m0, m1 = GPT2(_tiny(0.0)), GPT2(_tiny(0.0, 0.2))
    m1.load_state_dict(m0.state_dict())
    x, y = _batch(m0.cfg)
    loss = m1(x, y)
    assert torch.isfinite(loss) and not torch.equal(loss, m0(x, y))
    assert torch.equal(m1.eval()(x, y), m0.eval()(x, y))


def test_resume_reproduces_the_next_step():
    cfg = _tiny(0.1)
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
    assert tr2.drop_step == 2
    assert float(tr2.step(*batches[2]).detach()) == want
    # a checkpoint from before drop_step existed: loads, the stream starts at the resumed step
    old = {k: v for k, v in st.items() if k != "drop_step"}
    tr3 = GPT2Trainer(cfg, 2, 32, dev, dtype=torch.float32, dropout_seed=5)
    tr3.load_state_dict(old, 2)
    assert tr3.drop_step == 2 and float(tr3.step(*batches[2]).detach()) == want
    tr4 = GPT2Trainer(cfg, 2, 32, dev, dtype=torch.float32, dropout_seed=5)
    tr4.load_state_dict(old)
    assert tr4.drop_step == 0
    # another dropout seed draws other masks
    tr5 = GPT2Trainer(cfg, 2, 32, dev, dtype=torch.float32, dropout_seed=6)
    tr5.load_state_dict(st)
    assert float(tr5.step(*batches[2]).detach()) != want


def free_port_block(n=40):
    """A base port p with p..p+n free (best effort), below the ephemeral range."""
    import random
    import socket
    import time
    rng = random.Random(os.getpid() ^ time.time_ns())
    for _ in range(200):
        p = rng.randrange(12000, 32000 - n)
        try:
            for q in range(p, p + n):
                with socket.socket() as t:
                    t.bind(("127.0.0.1", q))
        except OSError:
            continue
        return p
    raise RuntimeError("no free port block")


def _launch(args, port):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=REPO, PDO_OPS="torch", POD_IP="127.0.0.1",
               PADDLE_PORT=str(port), CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-m", "paddle_operator_amd.launch", "--workload", "gpt2", "--tiny",
                          "--seq", "32", "--log-every", "1"] + args,
                         env=env, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _records(text, tag):
    return [json.loads(l[len(tag) + 1:]) for l in text.splitlines() if l.startswith(tag + " ")]


def test_launcher_flags():
    from paddle_operator_amd.launch.run import parse_args
    a = parse_args(["--workload", "gpt2", "--dropout", "0.1", "--attn-dropout", "0.05"])
    assert a.dropout == 0.1 and a.attn_dropout == 0.05
    a = parse_args(["--workload", "gpt2"])
    assert a.dropout == 0.0 and a.attn_dropout == 0.0
    done = _records(_launch(["--steps", "2", "--dropout", "0.1"], free_port_block()), "PDO_DONE")
    assert done and done[0]["steps"] == 2 and done[0]["dropout"] == 0.1 and done[0]["attn_dropout"] == 0.0
    bench = _records(_launch(["--steps", "1", "--warmup", "1", "--bench", "--dropout", "0.25"], free_port_block()),
                     "PDO_BENCH")
    assert bench and bench[0]["dropout"] == 0.25 and bench[0]["loss"] == bench[0]["loss"]
    bench0 = _records(_launch(["--steps", "1", "--bench"], free_port_block()), "PDO_BENCH")
    assert bench0 and bench0[0]["dropout"] == 0.0  # the default declares the headline's setting
