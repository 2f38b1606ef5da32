#!/usr/bin/env python3
"""LARS against momentum SGD on ResNet-50's arena, interleaved in one process.

* kernels: ``lars_flat`` (csrc/hip/lars.hip, three launches: 8 B per element read by the
  norm pass + 20 B moved by the update) against ``sgd_flat`` (20 B per element), on the
  arena and tensor table of the real model, with achieved TB/s;
* ``--step``: the batch-256 HIP-graph training step with ``optimizer="lars"`` against the
  SGD step, two trainers alive side by side, timed alternately.

    python tools/lars_probe.py [--rounds 3] [--step] [--batch 256] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernels(rounds):
    import torch

    from paddle_operator_amd import _native
    from paddle_operator_amd.models.resnet import resnet50
    from paddle_operator_amd.parallel.flat import FlatParams
    from paddle_operator_amd.workloads.resnet import FlatLARS, FlatSGD
    from tools.attn_probe import bench
    _native.require_hip()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    flat = FlatParams(resnet50(1000).to(dev), dtype=torch.float32, device=dev)
    flat.param_grads.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    for s in flat.slots:  # keep the padding zero
        end = -(-(s.offset + s.numel) // 1024) * 1024
        flat.param_grads[s.offset + s.numel:end] = 0
    opts = {"sgd": FlatSGD(flat, lr=1e-6), "lars": FlatLARS(flat, lr=1e-6)}
    ts = {k: [] for k in opts}
    for _ in range(rounds):
        for k, o in opts.items():
            ts[k].append(bench(lambda: o.step(0.125), iters=50, warm=5))
    n = flat.numel
    for k, b in (("sgd", 20), ("lars", 28)):
        print(json.dumps({"kernel": k + "_flat", "elements": n, "tensors": len(flat.slots), "us": [round(t, 1) for t in ts[k]],
                          "TBps": [round(b * n / t / 1e6, 2) for t in ts[k]], "bytes_per_element": b}), flush=True)


def step(rounds, batch, steps):
    import torch

    from paddle_operator_amd.workloads.resnet import ResNetTrainer
    tr = {}
    for k in ("sgd", "lars"):
        torch.manual_seed(0)
        tr[k] = ResNetTrainer(batch, "cuda:0", graph=True, optimizer=k)
        for _ in range(5):  # two eager steps, the capture, two replays
            tr[k].step()
        assert tr[k]._graph is not None
    ms = {k: [] for k in tr}
    for _ in range(rounds):
        for k, t in tr.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = t.step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
            assert bool(torch.isfinite(loss))
    for k in tr:
        print(json.dumps({"step": k, "batch": batch, "ms": [round(x, 3) for x in ms[k]],
                          "img_per_s": [round(batch / x * 1e3, 1) for x in ms[k]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    kernels(a.rounds)
    if a.step:
        step(a.rounds, a.batch, a.steps)


if __name__ == "__main__":
    main()
