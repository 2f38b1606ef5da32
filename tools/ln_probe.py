#!/usr/bin/env python3
"""LayerNorm kernels at the GPT-2-medium step's shape (65536 × 1024 bf16):
forward, backward, and the backward with the residual gradient joined and the
folded bias's column sum (the step's ``ln_bwd_kernel<2, true, 3>``), the fused
add + LayerNorm forward, the embedding forward, and the DROP instantiation of
each (counter-based dropout, p = 0.1); µs per call (median of rounds) and the
HBM bytes each moves per µs.

    python tools/ln_probe.py [--rows 65536] [--cols 1024] [--iters 20] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    from paddle_operator_amd import _native
    m = _native.require_hip()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    bf = dict(device=dev, dtype=torch.bfloat16)
    N, C = a.rows, a.cols
    x, dy, dres = (torch.randn(N, C, **bf) for _ in range(3))
    w, b = torch.randn(C, **bf), torch.randn(C, **bf)
    _, mean, rstd = m.layernorm_fwd(x, w, b, 1e-5)
    e = 2 * N * C  # bytes of one [N, C] bf16 tensor
    drop = dict(thr=6554, seed=0x9E3779B97F4A7C15, site=1, step=1)  # p = 0.1
    S = 1024 if N % 1024 == 0 else N
    idx = torch.randint(0, 50257, (N // S, S), device=dev)
    wte, wpe = torch.randn(50304, C, **bf), torch.randn(S, C, **bf)
    cases = {
        "ln_fwd": (lambda: m.layernorm_fwd(x, w, b, 1e-5), 2 * e),
        "ln_bwd": (lambda: m.layernorm_bwd(dy, x, w, mean, rstd), 3 * e),
        "ln_bwd_add_rbias": (lambda: m.layernorm_bwd_add(dy, x, w, mean, rstd, dres, True), 4 * e),
        "ln_bwd_add_rbias_drop": (lambda: m.layernorm_bwd_add(dy, x, w, mean, rstd, dres, True, **drop), 5 * e),
        "add_ln_fwd_rbias": (lambda: m.add_layernorm_fwd(x, dres, w, b, 1e-5, b), 4 * e),
        "add_ln_fwd_rbias_drop": (lambda: m.add_layernorm_fwd(x, dres, w, b, 1e-5, b, **drop), 4 * e),
        "embed_fwd": (lambda: m.embed_fwd(idx, wte, wpe), 2 * e),
        "embed_fwd_drop": (lambda: m.embed_fwd(idx, wte, wpe, **drop), 2 * e),
    }

    def timeit(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3

    res = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, (fn, _) in cases.items():
            res[k].append(timeit(fn))
    for k, (_, nbytes) in cases.items():
        us = statistics.median(res[k])
        print(json.dumps({"kernel": k, "rows": N, "cols": C, "us": round(us, 1), "TB_per_s": round(nbytes / us / 1e6, 2)}))


if __name__ == "__main__":
    main()
