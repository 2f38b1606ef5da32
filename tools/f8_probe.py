"""The FP8 QKV forward product against the bf16 one, in one process and interleaved rounds (median of
--rounds × --iters, device events): gemm_nt_f8 alone, the quantiser (amax + convert) of the activation and of
the weight, the whole quantise + GEMM call as ops.linear_fp8 issues it, and gemm_nt4 on the same product.
Shapes: [tokens, C] → 3C for C = 768, 1024, 1280 (GPT-2 small / medium / large QKV projections).

    python tools/f8_probe.py [--tokens 65536] [--iters 20] [--rounds 3] [--widths 768,1024,1280]

Numerics per shape: the largest |fp8 − bf16| output difference relative to the output's rms.

The same run also times what ``--fp8 ln`` adds (profiles/fp8_ln.md): the LayerNorm forward with and without the
e4m3 rows (q8), gemm_nt_f8 on per-token scales against the scalar form, fc1 (C → 4C) on gemm_nt_f8_gelu against
gemm_nt4's saved-gelu' epilogue, and the net per layer of each product = (LayerNorm q8 − LayerNorm) + quantise W +
FP8 GEMM − bf16 GEMM.

And what ``--fp8 lnmx`` adds (profiles/fp8_mx.md): fc1 on gemm_nt_f8_gelu with the MXFP8 copy of its output
(f8_fc1_mx against f8_fc1), fc2 (4C → C, bias + residual epilogue) on gemm_nt_mx8 against gemm_nt4, and the net per
layer = (f8_fc1_mx − f8_fc1) + quantise W2 + mx8_fc2 − nt4_fc2.

    python tools/f8_probe.py --step 64 [--model gpt2-medium] [--steps 8] [--rounds 3]   # step time, off / qkv / ln / lnmx
    python tools/f8_probe.py --losses 40 [--micro-batch 8]                              # losses of the modes

    python tools/f8_probe.py --wq 64 [--grad-accum 1] [--model gpt2-medium] [--steps 8] [--rounds 3]   # profiles/fp8_wq.md

--wq: the step's e4m3 weights from the arena (FlatParams.enable_wq) against just in time, for fp8 = ln and lnmx: the
grouped launch pair over the mode's whole weight set against the summed per-tensor quant_e4m3 calls it replaces
(device events), then the step time with ops.fp8._WQ_ARENA off and on in interleaved rounds on one trainer, and the
peak device memory without and with the byte arena.  The per-width rows carry quant_w_grouped: one layer's three
weights in one grouped pair, beside quant_w + quant_w1 + quant_w2.

--step: one trainer, GPT2Config.fp8 switched between rounds (host clock around a device synchronise, warm-up for
every mode).  --losses: a fresh trainer per mode, same seed, synthetic stream, lr 3e-4.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_operator_amd import _native  # noqa: E402


def bench(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


MODES = ("off", "qkv", "ln", "lnmx")


def _trainer(model, micro_batch, seq):
    from paddle_operator_amd.models.gpt2 import GPT2Config
    from paddle_operator_amd.train import GPT2Trainer
    return GPT2Trainer(GPT2Config.named(model), micro_batch, seq, torch.device("cuda", 0), lr=3e-4, seed=0)


def step_times(a):
    import time
    tr = _trainer(a.model, a.step, a.seq)
    times = {k: [] for k in MODES}
    for rnd in range(a.rounds + 1):  # round 0: warm-up of every mode
        for k in MODES:
            tr.cfg.fp8 = k
            for _ in range(3 if rnd == 0 else 1):  # one untimed step after every switch
                tr.step()
            if rnd == 0:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    rec = {"model": a.model, "micro_batch": a.step, "seq": a.seq, "steps": a.steps}
    for k, v in times.items():
        rec[k + "_ms"] = [round(t, 3) for t in v]
        rec[k + "_median_ms"] = round(statistics.median(v), 3)
    print(json.dumps(rec), flush=True)


def _grouped(m, ws):
    """(call, elements): the grouped quantiser over the bf16 matrices ``ws`` laid out as one arena."""
    from paddle_operator_amd.parallel.flat import ALIGN, wq_table
    segs, off = [], 0
    for w in ws:
        segs.append((off, w.numel()))
        off = (off + w.numel() + ALIGN - 1) // ALIGN * ALIGN
    arena = torch.zeros(off, device=ws[0].device, dtype=torch.bfloat16)
    for (o, n), w in zip(segs, ws):
        arena[o:o + n] = w.reshape(-1)
    rows, chunks, nbytes = wq_table(segs)
    host = torch.tensor(rows, dtype=torch.int64)
    dev = host.to(arena.device)
    q = torch.empty(nbytes, device=arena.device, dtype=torch.uint8)
    amax = torch.zeros(len(rows), device=arena.device, dtype=torch.int32)
    d = torch.zeros(len(rows), device=arena.device)
    return (lambda: m.quant_e4m3_grouped(arena, q, amax, d, dev, host, chunks)), sum(n for _, n in segs)


def wq_times(a):
    import gc
    import time
    from paddle_operator_amd.models.gpt2 import GPT2Config
    from paddle_operator_amd.ops import fp8
    from paddle_operator_amd.train import GPT2Trainer, fp8_weights
    m = _native.require_hip()
    dev = torch.device("cuda", 0)
    for mode in ("ln", "lnmx"):
        rec = {"model": a.model, "fp8": mode, "micro_batch": a.wq, "grad_accum": a.grad_accum, "seq": a.seq, "steps": a.steps}
        mem = {}
        for arena in (False, True):  # without: built with fp8 off, the mode set afterwards (no enable_wq)
            gc.collect()  # the previous trainer (its parameters point back at its arena) before its blocks are reused
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            cfg = GPT2Config.named(a.model)
            cfg.fp8 = mode if arena else "off"
            tr = GPT2Trainer(cfg, a.wq, a.seq, dev, lr=3e-4, seed=0, grad_accum=a.grad_accum)
            tr.cfg.fp8 = mode
            for _ in range(3):
                tr.step()
            torch.cuda.synchronize()
            mem[arena] = torch.cuda.max_memory_allocated() / 2 ** 30
            if not arena:
                tr.close()
                del tr
        rec["max_mem_gb_without"], rec["max_mem_gb_with"] = round(mem[False], 3), round(mem[True], 3)
        rec["arena_gb"] = round(tr.flat.wq.numel() / 2 ** 30, 3)
        # the kernels: the trainer's own table against one quant_e4m3 per covered weight
        ws = fp8_weights(tr.model, mode)
        n = sum(w.numel() for w in ws)
        fl = tr.flat
        fns = {"grouped": lambda: m.quant_e4m3_grouped(fl.params, fl.wq, fl.wq_amax, fl.wq_dscale, fl._wq_dev, fl._wq_host,
                                                       fl._wq_chunks),
               "per_tensor": lambda: [m.quant_e4m3(w) for w in ws]}
        kt = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                kt[k].append(bench(fn, a.iters))
        rec["tensors"], rec["elements"] = len(ws), n
        for k, v in kt.items():
            rec[k + "_us"] = [round(t, 1) for t in v]
        # bytes the pair needs: two reads of the bf16 values and one write of the bytes
        rec["grouped_TBps"] = round(5.0 * n / statistics.median(kt["grouped"]) / 1e6, 3)
        times, peak = {False: [], True: []}, {False: [], True: []}
        for rnd in range(a.rounds + 1):  # round 0: warm-up of both
            for hook in (False, True):
                fp8._WQ_ARENA[0] = hook
                tr.step()
                if rnd == 0:
                    continue
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    tr.step()
                torch.cuda.synchronize()
                times[hook].append((time.perf_counter() - t0) / a.steps * 1e3)
                peak[hook].append(round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))
        fp8._WQ_ARENA[0] = True
        rec["jit_ms"], rec["arena_ms"] = ([round(t, 3) for t in times[h]] for h in (False, True))
        # the same trainer (byte arena allocated either way): what the path alone does to the peak
        rec["jit_peak_gb"], rec["arena_peak_gb"] = peak[False], peak[True]
        print(json.dumps(rec), flush=True)
        tr.close()
        del tr, ws, fl, fns


def losses(a):
    for k in MODES:
        tr = _trainer(a.model, a.micro_batch, a.seq)
        tr.cfg.fp8 = k
        ls = [float(tr.step().detach()) for _ in range(a.losses)]
        print(json.dumps({"fp8": k, "micro_batch": a.micro_batch, "step_1": round(ls[0], 6), "last": round(ls[-1], 6),
                          "mean_last_5": round(sum(ls[-5:]) / 5, 6)}), flush=True)
        tr.close()
        del tr
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--widths", default="768,1024,1280")
    ap.add_argument("--step", type=int, default=0, metavar="MICRO_BATCH", help="time the training step instead")
    ap.add_argument("--losses", type=int, default=0, metavar="STEPS", help="print the modes' losses instead")
    ap.add_argument("--wq", type=int, default=0, metavar="MICRO_BATCH", help="time the step's e4m3 weight arena instead")
    ap.add_argument("--grad-accum", type=int, default=1)
    ap.add_argument("--model", default="gpt2-medium")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--micro-batch", type=int, default=8)
    a = ap.parse_args()
    if a.step:
        return step_times(a)
    if a.losses:
        return losses(a)
    if a.wq:
        return wq_times(a)
    m = _native.require_hip()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    M = a.tokens
    for C in (int(c) for c in a.widths.split(",")):
        N, K = 3 * C, C
        if not m.gemm_nt_f8_supported(M, N, K):
            raise SystemExit(f"gemm_nt_f8 does not take {M} x {N} x {K}")
        x = torch.empty(M, K, device=dev, dtype=torch.bfloat16).normal_(0, 1, generator=g)
        w = torch.empty(N, K, device=dev, dtype=torch.bfloat16).normal_(0, 0.02, generator=g)
        b = torch.empty(N, device=dev, dtype=torch.bfloat16).uniform_(-0.1, 0.1, generator=g)
        (qx, dx), (qw, dw) = m.quant_e4m3(x), m.quant_e4m3(w)

        def whole():
            (q1, d1), (q2, d2) = m.quant_e4m3(x), m.quant_e4m3(w)
            return m.gemm_nt_f8(q1, d1, q2, d2, b)

        # --fp8 ln: x stands for the LayerNorm's input as well; its own rows and per-token scales feed the row form
        lw, lb = torch.ones(K, device=dev, dtype=torch.bfloat16), torch.zeros(K, device=dev, dtype=torch.bfloat16)
        qr, dr = m.layernorm_fwd(x, lw, lb, 1e-5, True)[-2:]
        w1 = torch.empty(4 * C, K, device=dev, dtype=torch.bfloat16).normal_(0, 0.02, generator=g)
        b1 = torch.empty(4 * C, device=dev, dtype=torch.bfloat16).uniform_(-0.1, 0.1, generator=g)
        qw1, dw1 = m.quant_e4m3(w1)
        # --fp8 lnmx: fc2 from the MXFP8 rows of fc1's output, bias and residual (x) in the epilogue
        w2 = torch.empty(C, 4 * C, device=dev, dtype=torch.bfloat16).normal_(0, 0.02, generator=g)
        b2 = torch.empty(C, device=dev, dtype=torch.bfloat16).uniform_(-0.1, 0.1, generator=g)
        _, h, qh, sh = m.gemm_nt_f8_gelu(qr, dr, qw1, dw1, b1, mx=True)
        qw2, dw2 = m.quant_e4m3(w2)
        grouped, _ = _grouped(m, [w, w1, w2])

        fns = {"quant_w_grouped": grouped,  # one layer's three weights: against quant_w + quant_w1 + quant_w2
               "f8_gemm": lambda: m.gemm_nt_f8(qx, dx, qw, dw, b), "quant_x": lambda: m.quant_e4m3(x),
               "quant_w": lambda: m.quant_e4m3(w), "f8_whole": whole, "nt4": lambda: m.gemm_nt(x, w, b),
               "ln": lambda: m.layernorm_fwd(x, lw, lb, 1e-5), "ln_q8": lambda: m.layernorm_fwd(x, lw, lb, 1e-5, True),
               "f8_rows": lambda: m.gemm_nt_f8(qr, dr, qw, dw, b), "quant_w1": lambda: m.quant_e4m3(w1),
               "f8_fc1": lambda: m.gemm_nt_f8_gelu(qr, dr, qw1, dw1, b1),
               "nt4_fc1": lambda: m.gemm_nt_gelu(x, w1, b1, saved_grad=True),
               "f8_fc1_mx": lambda: m.gemm_nt_f8_gelu(qr, dr, qw1, dw1, b1, mx=True), "quant_w2": lambda: m.quant_e4m3(w2),
               "mx8_fc2": lambda: m.gemm_nt_mx8(qh, sh, qw2, dw2, b2, x), "nt4_fc2": lambda: m.gemm_nt_add(h, w2, x, bias=b2)}
        y8, y16 = whole().float(), m.gemm_nt(x, w, b).float()
        rel = ((y8 - y16).abs().max() / y16.pow(2).mean().sqrt()).item()
        del y8, y16
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(bench(fn, a.iters))
        fl = 2.0 * M * N * K
        rec = {"C": C, "M": M, "N": N, "K": K, "max_diff_over_rms": round(rel, 4)}
        for k, v in times.items():
            rec[k + "_us"] = round(statistics.median(v), 1)
            rec[k + "_spread_us"] = round(max(v) - min(v), 1)
        for k in ("f8_gemm", "f8_whole", "nt4"):
            rec[k + "_PF"] = round(fl / rec[k + "_us"] / 1e9, 3)
        rec["net_us_per_layer"] = round(rec["f8_whole_us"] - rec["nt4_us"], 1)  # < 0: the FP8 call is faster
        ln_extra = rec["ln_q8_us"] - rec["ln_us"]  # paid once per LayerNorm, i.e. once per product
        rec["ln_net_qkv_us"] = round(ln_extra + rec["quant_w_us"] + rec["f8_rows_us"] - rec["nt4_us"], 1)
        rec["ln_net_fc1_us"] = round(ln_extra + rec["quant_w1_us"] + rec["f8_fc1_us"] - rec["nt4_fc1_us"], 1)
        rec["mx8_fc2_PF"] = round(2.0 * M * C * 4 * C / rec["mx8_fc2_us"] / 1e9, 3)
        rec["mx_net_fc2_us"] = round(rec["f8_fc1_mx_us"] - rec["f8_fc1_us"] + rec["quant_w2_us"] + rec["mx8_fc2_us"]
                                     - rec["nt4_fc2_us"], 1)
        print(json.dumps(rec), flush=True)
        del x, w, b, qx, qw, qr, dr, w1, b1, qw1, w2, b2, h, qh, sh, qw2


if __name__ == "__main__":
    main()
