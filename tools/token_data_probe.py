#!/usr/bin/env python3
"""Step cost of token-file training (profiles/r11_token_data.md).

One process, one GPU: a synthetic-batch trainer, a trainer on a device-resident
corpus and one on a host-staged corpus, run alternately for ``--rounds`` rounds
of ``--steps`` steps (the step A/B convention: same process, interleaved); then
``--grad-accum`` micro-batches per step with the fp32 accumulator, the
``grad_accum_fold`` kernel alone under device events, and peak memory with and
without the accumulator.  The corpus is random ids written to a temporary file.

    python tools/token_data_probe.py --model gpt2-medium --batch 32 --out r11.json
"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_operator_amd import _native  # noqa: E402
from paddle_operator_amd.models.gpt2 import GPT2Config  # noqa: E402
from paddle_operator_amd.train import GPT2Trainer  # noqa: E402


def timed(tr, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-medium")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grad-accum", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=64 << 20, help="corpus length")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("token_data_probe: needs a GPU")  # a CPU timing says nothing about the step
    dev = torch.device("cuda", 0)
    cfg = GPT2Config.named(a.model)
    B, S, K = a.batch, a.seq, a.grad_accum
    out = {"model": a.model, "B": B, "S": S, "gpu": torch.cuda.get_device_name(0), "corpus_tokens": a.tokens}
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "train.bin")
    np.random.default_rng(0).integers(0, cfg.vocab_size, a.tokens).astype("<u2").tofile(path)
    try:
        variants = {"synthetic": {}, "device": dict(data=path), "host": dict(data=path, data_device_gb=0.0)}
        trainers = {k: GPT2Trainer(cfg, B, S, dev, **kw) for k, kw in variants.items()}
        for tr in trainers.values():
            timed(tr, a.warmup)
        rounds = {k: [] for k in trainers}
        for r in range(a.rounds):
            for k, tr in trainers.items():
                rounds[k].append(round(timed(tr, a.steps), 3))
            print("round", r, {k: v[-1] for k, v in rounds.items()}, flush=True)
        out["step_ms"] = rounds
        for tr in trainers.values():
            tr.check_data()
            tr.close()
        del trainers, tr
        for k, key in ((1, "max_mem_gb_K1"), (K, f"max_mem_gb_K{K}")):
            gc.collect()  # the previous trainer's cycles, so that its arenas are not in this peak
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            tr = GPT2Trainer(cfg, B, S, dev, data=path, grad_accum=k)
            timed(tr, 1)
            if k > 1:
                acc_ms = [round(timed(tr, 3), 3) for _ in range(a.rounds)]
                out["accum_step_ms"] = acc_ms
                out["accum_ms_per_micro_batch"] = [round(t / k, 3) for t in acc_ms]
            out[key] = round(torch.cuda.max_memory_allocated(dev) / 2**30, 2)
            if k == 1:
                tr.close()
                del tr
        out["grad_accum"] = K
        out["grad_elements"] = n = tr.flat.grads.numel()
        if tr.acc is not None:
            m = _native.require_hip()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                m.grad_accum_fold(tr.flat.grads, tr.acc, False, False)
            e0.record()
            for _ in range(20):
                m.grad_accum_fold(tr.flat.grads, tr.acc, False, False)
            e1.record()
            torch.cuda.synchronize()
            fold = e0.elapsed_time(e1) / 20
            out["fold_ms"] = round(fold, 4)
            out["fold_GBps"] = round(n * 12 / fold / 1e6, 1)  # per element: 2 + 4 B read, 4 + 2 B written
            out["fold_share_of_accum_step"] = round((K - 1) * fold / min(out["accum_step_ms"]), 5)
        tr.close()
    finally:
        os.remove(path)
        os.rmdir(tmp)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
