"""Wide&Deep / DeepFM training step on one GPU: the HIP sparse path against the
framework path (``PDO_OPS=torch``), interleaved in one process.

    python tools/bench_ctr.py [--models wide_deep,deepfm] [--batches 4096,32768]
                              [--rounds 3] [--steps 20] [--warmup 5] [--out FILE] [--data DIR]

Per model and batch: two ``CTRTrainer``s (same seeds, same batches), one built and
stepped with ``PDO_OPS=hip``, one with ``PDO_OPS=torch``; each round times ``--steps``
steps of one, then of the other (device events around the loop).  Then ``ctr_fwd``
and ``ctr_bwd_rows`` alone (device events, 50 launches each, the sort outside), with
the bytes each moves.  One JSON line per (model, batch).

``--data DIR`` (a click directory, ``paddle_operator_amd.data.CLICK_DOC``) adds a third
arm to the same rounds: the HIP step fed from the directory, device-resident
(``files_device``) and host-staged (``files_host``); the synthetic ``hip`` arm is their
yardstick.  Then ``click_batch`` alone, with its bytes, next to the synthetic draw.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernels_alone(torch, tr, launches=50):
    """µs and bytes of the two kernels on the trainer's tables and one of its batches."""
    from paddle_operator_amd import _native
    from paddle_operator_amd.ops import ctr as ops
    hip = _native.require_hip()
    ids, dense, _ = tr.draw(0, 0)
    B, S = ids.shape
    D, nd, N = tr.cfg.emb_dim, tr.cfg.n_dense, B * S
    us_fwd = timed(torch, lambda: hip.ctr_fwd(ids, dense, tr.deep, tr.wide, tr.ldx, tr.fm), launches) * 1e3
    X, ws, fmt, ssum = ops.ctr_lookup(ids, dense, tr.deep, tr.wide, tr.fm, tr.ldx)
    dX, dlogit = torch.randn_like(X) * 1e-4, torch.randn_like(ws) * 1e-4
    keys, perm = torch.sort(ids.reshape(-1), stable=True)
    deep, wide, acc_d, acc_w = (t.clone() for t in (tr.deep, tr.wide, tr.deep_acc, tr.wide_acc))
    us_bwd = timed(torch, lambda: hip.ctr_bwd_rows(keys, perm, dX, dlogit, ssum if tr.fm else None, S, deep, wide,
                                                   acc_d, acc_w, tr.lr_dev, 1), launches) * 1e3
    us_sort = timed(torch, lambda: torch.sort(ids.reshape(-1), stable=True), launches) * 1e3
    uniq = int(torch.unique(ids).numel())
    fm_b = B * D * 4 + B * 4 if tr.fm else 0
    bytes_fwd = N * 8 + N * (D + 1) * 4 + B * nd * 4 + B * tr.ldx * 4 + B * 4 + fm_b
    # keys + perm, a dX row and dlogit per lookup (ssum too with fm), and w, acc read and written per touched row
    bytes_bwd = N * 16 + N * D * 4 + N * 4 + (N * D * 4 if tr.fm else 0) + uniq * (D + 1) * 4 * 4
    return {"ctr_fwd_us": round(us_fwd, 1), "ctr_fwd_bytes": bytes_fwd,
            "ctr_fwd_GBps": round(bytes_fwd / us_fwd / 1e3, 1), "ctr_bwd_rows_us": round(us_bwd, 1),
            "ctr_bwd_rows_bytes": bytes_bwd, "ctr_bwd_rows_GBps": round(bytes_bwd / us_bwd / 1e3, 1),
            "sort_us": round(us_sort, 1), "lookups": N, "rows_touched": uniq}


def click_batch_alone(torch, tr, launches=50):
    """µs and bytes of ``click_batch`` on the trainer's device-resident click set: per row it reads
    S uint32, n_dense int32 and a label byte and writes S int64, n_dense fp32 and an fp32 label."""
    s = tr.train
    us = timed(torch, lambda: s.batch(3), launches) * 1e3
    nbytes = s.B * (s.S * (4 + 8) + s.n_dense * (4 + 4) + 1 + 4)
    return {"click_batch_us": round(us, 1), "click_batch_bytes": nbytes, "click_batch_GBps": round(nbytes / us / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="",
                    help="click directory (tools/criteo_to_clicks.py): adds the file-fed HIP step, device-resident "
                         "(files_device) and host-staged (files_host), to the interleaved rounds")
    ap.add_argument("--models", default="wide_deep,deepfm")
    ap.add_argument("--batches", default="4096,32768")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from paddle_operator_amd.models.wide_deep import WideDeepConfig
    from paddle_operator_amd.workloads.ctr import CTRTrainer
    lines = []
    for model in a.models.split(","):
        for batch in (int(b) for b in a.batches.split(",")):
            trainers = {}
            # with --data: the HIP step fed from the click directory, device-resident and host-staged
            arms = {"hip": {}, "torch": {}}
            if a.data:
                arms["files_device"] = {"data": a.data, "data_device_gb": 1e6}
                arms["files_host"] = {"data": a.data, "data_device_gb": 0.0}
            for mode, kw in arms.items():
                os.environ["PDO_OPS"] = "torch" if mode == "torch" else "hip"
                trainers[mode] = CTRTrainer(WideDeepConfig(model=model), batch, "cuda:0", **kw)
                for _ in range(a.warmup):
                    trainers[mode].step()
            torch.cuda.synchronize()
            ms = {mode: [] for mode in arms}
            for _ in range(a.rounds):
                for mode in arms:
                    os.environ["PDO_OPS"] = "torch" if mode == "torch" else "hip"
                    ms[mode].append(round(timed(torch, trainers[mode].step, a.steps), 3))
            loss = {}
            for mode in ("torch", "hip"):  # the same step count on both: the losses are comparable
                os.environ["PDO_OPS"] = mode
                loss[mode] = float(trainers[mode].step())
            rec = {"model": model, "batch": batch, "gpu": torch.cuda.get_device_name(0), "steps": a.steps,
                   "step_ms": ms, "samples_per_s": {m: [round(batch / t * 1e3) for t in v] for m, v in ms.items()},
                   "hip_faster_every_round": all(h < t for h, t in zip(ms["hip"], ms["torch"])), "loss": loss}
            rec.update(kernels_alone(torch, trainers["hip"]))
            if a.data:
                rec.update(click_batch_alone(torch, trainers["files_device"]))
                rec["synthetic_draw_us"] = round(timed(torch, lambda: trainers["hip"].draw(0, 3), 50) * 1e3, 1)
                rec["click_records"] = trainers["files_device"].train.n
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            for t in trainers.values():
                t.close()
            del trainers
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
