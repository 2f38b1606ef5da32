"""The FP8 QKV forward product against the bf16 one, in one process and interleaved rounds (median of
--rounds × --iters, device events): gemm_nt_f8 alone, the quantiser (amax + convert) of the activation and of
the weight, the whole quantise + GEMM call as ops.linear_fp8 issues it, and gemm_nt4 on the same product.
Shapes: [tokens, C] → 3C for C = 768, 1024, 1280 (GPT-2 small / medium / large QKV projections).

    python tools/f8_probe.py [--tokens 65536] [--iters 20] [--rounds 3] [--widths 768,1024,1280]

Numerics per shape: the largest |fp8 − bf16| output difference relative to the output's rms.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--widths", default="768,1024,1280")
    a = ap.parse_args()
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

        fns = {"f8_gemm": lambda: m.gemm_nt_f8(qx, dx, qw, dw, b), "quant_x": lambda: m.quant_e4m3(x),
               "quant_w": lambda: m.quant_e4m3(w), "f8_whole": whole, "nt4": lambda: m.gemm_nt(x, w, b)}
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
        print(json.dumps(rec), flush=True)
        del x, w, b, qx, qw


if __name__ == "__main__":
    main()
