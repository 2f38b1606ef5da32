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
    ap.add_argument("--model", default="gpt2-medium")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--micro-batch", type=int, default=8)
    a = ap.parse_args()
    if a.step:
        return step_times(a)
    if a.losses:
        return losses(a)
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

        fns = {"f8_gemm": lambda: m.gemm_nt_f8(qx, dx, qw, dw, b), "quant_x": lambda: m.quant_e4m3(x),
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
