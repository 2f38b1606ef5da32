#!/usr/bin/env python3
"""Step cost of ResNet-50 on image files (profiles/r14_image_data.md).

One process, one GPU: a synthetic-batch trainer, one on a device-resident image set and
one on a host-staged set, run alternately for ``--rounds`` rounds of ``--steps`` steps
(the step A/B convention: same process, interleaved); then the ``image_batch`` kernel
alone under device events with its byte traffic, the gather thread pool alone, and one
``evaluate()`` over ``--eval-images`` images.  The sets are random pixels written to a
temporary directory.

    python tools/image_data_probe.py --batch 256 --out r14.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_operator_amd.workloads.resnet import ResNetTrainer  # noqa: E402


def timed(tr, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def write_set(path, n, R, seed):
    os.makedirs(path)
    rng = np.random.default_rng(seed)
    img = np.lib.format.open_memmap(os.path.join(path, "images.npy"), "w+", np.uint8, (n, R, R, 3))
    for o in range(0, n, 512):
        img[o:o + 512] = rng.integers(0, 256, img[o:o + 512].shape, dtype=np.uint8)
    img.flush()
    np.save(os.path.join(path, "labels.npy"), rng.integers(0, 1000, n).astype(np.int16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=2048, help="training set size")
    ap.add_argument("--side", type=int, default=256, help="stored side R")
    ap.add_argument("--eval-images", type=int, default=10000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_data_probe: needs a GPU")  # a CPU timing says nothing about the step
    dev = torch.device("cuda", 0)
    B, R = a.batch, a.side
    out = {"B": B, "R": R, "gpu": torch.cuda.get_device_name(0), "images": a.images}
    tmp = tempfile.mkdtemp()
    train, val = os.path.join(tmp, "train"), os.path.join(tmp, "val")
    try:
        write_set(train, a.images, R, 0)
        write_set(val, a.eval_images, R, 1)
        variants = {"synthetic": {}, "device": dict(data=train), "host": dict(data=train, data_device_gb=0.0)}
        trainers = {k: ResNetTrainer(B, dev, graph=True, **kw) for k, kw in variants.items()}
        for tr in trainers.values():
            timed(tr, a.warmup)
        rounds = {k: [] for k in trainers}
        for r in range(a.rounds):
            for k, tr in trainers.items():
                rounds[k].append(round(timed(tr, a.steps), 3))
            print("round", r, {k: v[-1] for k, v in rounds.items()}, flush=True)
        out["step_ms"] = rounds
        out["hip_graph"] = {k: tr._graph is not None for k, tr in trainers.items()}

        # image_batch alone: device-resident set, the trainer's own buffers
        tr = trainers["device"]
        xb, _, yb = tr._batch_buffers()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for m in range(3):
            tr.data.batch(m, out=(xb, yb))
        e0.record()
        for m in range(50):
            tr.data.batch(m, out=(xb, yb))
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 50 * 1e3
        boxes = np.concatenate([tr.data.boxes(m) for m in range(50)])
        rd = float((boxes[:, 3] * boxes[:, 4]).mean()) * 3 * B  # the crop's pixels, each byte once
        wr = B * tr.res * tr.res * 3 * 2 + B * 8
        out["image_batch_us"] = round(us, 1)
        out["image_batch_bytes"] = {"read_crop": int(rd), "written": wr}
        out["image_batch_GBps"] = round((rd + wr) / us / 1e3, 1)

        # the normal_() draw it replaces
        ts = trainers["synthetic"]
        xs, _, ys = ts._batch_buffers()
        e0.record()
        for _ in range(50):
            ts._draw(xs, ys)
        e1.record()
        torch.cuda.synchronize()
        out["synthetic_draw_us"] = round(e0.elapsed_time(e1) / 50 * 1e3, 1)

        # the host gather alone (page cache warm): what the staging thread pool sustains
        th = trainers["host"].data
        buf, lab = th._pinned[0].numpy(), th._pinned_lab[0].numpy()
        t0 = time.perf_counter()
        for m in range(100, 110):
            th._gather(th.boxes(m)[:, 0], buf, lab, None)
        one = (time.perf_counter() - t0) / 10
        out["gather_ms_1_thread"] = round(one * 1e3, 2)
        out["gather_GBps_1_thread"] = round(B * R * R * 3 / one / 1e9, 2)
        h2d = torch.empty_like(th._staged[0])
        e0.record()
        for _ in range(10):
            h2d.copy_(th._pinned[0], non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        out["h2d_ms"] = round(e0.elapsed_time(e1) / 10, 3)
        for t in trainers.values():
            t.close()
        del trainers, tr, ts, th

        # one evaluate() over the whole validation set, and the training forward for scale
        ev = ResNetTrainer(B, dev, val_data=val)
        ev.step()
        ev.evaluate(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.evaluate()
        dt = time.perf_counter() - t0
        out["evaluate"] = {"images": res["images"], "seconds": round(dt, 3),
                           "images_per_s": round(res["images"] / dt, 1), "batches": ev.val.batches_per_epoch()}
        x, _ = ev.batch()
        e0.record()
        for _ in range(5):
            with ev.flat.shadow_scope(), torch.autocast("cuda", dtype=torch.bfloat16):
                ev.model(x)
        e1.record()
        torch.cuda.synchronize()
        out["train_forward_ms"] = round(e0.elapsed_time(e1) / 5, 3)
        ev.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
