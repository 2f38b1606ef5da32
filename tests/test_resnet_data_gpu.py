"""ResNet-50 on image files on the MI355X: the captured step against the eager one with data and a
schedule, sgd_flat's device-resident rate, evaluate() against a recount, and the launcher's
PDO_EVAL records across a resume.  Every test writes its own small ``.npy`` sets under ``tmp_path``.
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xF234_5678_9ABC_DEF1


def _write_set(path, n, R, classes, seed):
    rng = np.random.default_rng(seed)
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "images.npy"), rng.integers(0, 256, (n, R, R, 3), dtype=np.uint8))
    np.save(os.path.join(path, "labels.npy"), rng.integers(0, classes, n).astype(np.int16))
    return str(path)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("resnet-data")
    return _write_set(d / "train", 64, 256, 1000, 1), _write_set(d / "val", 19, 256, 1000, 2)


def test_sgd_flat_lr_dev_equals_by_value(cuda):
    from paddle_operator_amd import _native
    m = _native.require_hip()
    n = 2048
    g = torch.Generator().manual_seed(0)
    w, gr, buf = (torch.randn(n, generator=g).to(cuda) for _ in range(3))
    dec = torch.tensor([1.0, 0.0], device=cuda)
    lr = 0.0737
    a = [t.clone() for t in (w, buf)]
    b = [t.clone() for t in (w, buf)]
    m.sgd_flat(a[0], gr, a[1], dec, lr, 0.9, 5e-5, 0.5)
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=cuda)
    m.sgd_flat(b[0], gr, b[1], dec, 123.0, 0.9, 5e-5, 0.5, lr_dev)  # the by-value rate is ignored
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], w)
    assert float(lr_dev) == float(np.float32(lr))


def test_graph_step_with_data_and_schedule_matches_eager(cuda, sets):
    """5 steps (2 eager, the capture, 2 replays) on a 64-image set at R = 256 with a cosine
    schedule: bitwise the eager trainer's losses, weights, momentum and running statistics, and the
    rate in the device tensor at every step is the shared formula's."""
    from paddle_operator_amd.ops.optim import cosine_lr
    from paddle_operator_amd.workloads.resnet import ResNetTrainer
    runs = []
    for graph in (False, True):
        torch.manual_seed(0)
        t = ResNetTrainer(8, cuda, graph=graph, data=sets[0], data_seed=SEED, lr=0.2, lr_schedule="cosine",
                          lr_warmup=2, lr_decay_steps=5, lr_min_ratio=0.1)
        assert t.data.placement == "device"
        losses, rates = [], []
        for _ in range(5):
            losses.append(float(t.step()))
            rates.append(float(t.lr_dev))
        torch.cuda.synchronize()
        bufs = torch.cat([b.float().flatten() for b in t.model.buffers()])
        runs.append((losses, rates, t.flat.params.clone(), t.opt.buf.clone(), bufs, t.opt.step_count,
                     t._graph is not None))
        t.close()
    (le, re_, pe, me, be, ne, ge), (lg, rg, pg, mg, bg, ng, gg) = runs
    assert not ge and gg, "graph mode not taken"
    assert ne == ng == 5 and le == lg, (le, lg)
    want = [float(np.float32(cosine_lr(s, 0.2, 2, 5, 0.1))) for s in range(5)]
    assert re_ == rg == want and len(set(want)) == 4, (re_, rg, want)  # (steps 1 and 2 both run at the peak)
    assert torch.equal(pe, pg) and torch.equal(me, mg) and torch.equal(be, bg)
    assert all(np.isfinite(le))


def test_evaluate_counts_and_leaves_training_untouched(cuda, sets):
    from paddle_operator_amd.ops import resnet as R
    from paddle_operator_amd.workloads.resnet import ResNetTrainer

    def run(evaluate):
        """Two eager steps and the capture, the evaluation (or not), one replayed step."""
        torch.manual_seed(0)
        t = ResNetTrainer(8, cuda, graph=True, data=sets[0], val_data=sets[1], data_seed=SEED)
        losses = [float(t.step()) for _ in range(3)]
        assert t._graph is not None
        if evaluate:
            evaluate(t)
        losses.append(float(t.step()))
        torch.cuda.synchronize()
        out = (losses, t.flat.params.clone(), t.opt.buf.clone(),
               torch.cat([b.float().flatten() for b in t.model.buffers()]), t.opt.step_count)
        t.close()
        return out

    def evaluation(a):
        stats = {k: v.clone() for k, v in a.model.named_buffers()}
        used0 = R._EVAL_USED[0]
        ev = a.evaluate()
        assert R._EVAL_USED[0] - used0 == 3 * 53  # every BatchNorm of every batch on the HIP eval kernels
        assert ev["images"] == 19 and set(ev) == {"val_loss", "top1", "top5", "images"}
        assert a.model.training and all(torch.equal(v, stats[k]) for k, v in a.model.named_buffers())
        # recount from the eval logits
        a.model.eval()
        loss = torch.zeros((), dtype=torch.float64, device=cuda)
        top1 = top5 = cnt = 0
        with torch.no_grad(), a.flat.shadow_scope(), torch.autocast("cuda", dtype=torch.bfloat16):
            for m in range(3):
                x, y = a.val.batch(m)
                out = a.model(x).float()
                ok = y >= 0
                loss += torch.nn.functional.cross_entropy(out[ok], y[ok], reduction="sum").double()
                top1 += int((out[ok].argmax(1) == y[ok]).sum())
                top5 += int((out[ok].topk(5, dim=1).indices == y[ok][:, None]).any(1).sum())
                cnt += int(ok.sum())
        a.model.train()
        assert cnt == 19 and ev["top1"] == top1 / 19 and ev["top5"] == top5 / 19
        assert abs(ev["val_loss"] - float(loss) / 19) <= 1e-6 * abs(ev["val_loss"])
        assert ev == a.evaluate()

    # the next (replayed) training step is bitwise what it is without the evaluation
    (la, pa, ma, ba, na), (lb, pb, mb, bb, nb) = run(evaluation), run(None)
    assert na == nb == 4 and la == lb, (la, lb)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(ba, bb)


def _launch(args, port):
    env = dict(os.environ, PYTHONPATH=REPO, POD_IP="127.0.0.1", PADDLE_PORT=str(port))
    out = subprocess.run([sys.executable, "-m", "paddle_operator_amd.launch", "--workload", "resnet50"] + args,
                         env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    def rec(tag):
        return [json.loads(l[len(tag) + 1:]) for l in out.stdout.splitlines() if l.startswith(tag + " ")]
    return rec("PDO_EVAL"), rec("PDO_DONE")


def test_launcher_eval_records_and_resume(cuda, sets, tmp_path):
    common = ["--data", sets[0], "--val-data", sets[1], "--data-seed", "7", "--eval-every", "2", "--steps", "4",
              "--batch", "8", "--lr-schedule", "cosine", "--lr-warmup", "1", "--ckpt-every", "2"]
    ev, done = _launch(common + ["--ckpt-dir", str(tmp_path / "ck")], 36530)
    assert [e["step"] for e in ev] == [2, 4], ev
    assert all(set(e) == {"step", "val_loss", "top1", "top5", "images"} and e["images"] == 19 for e in ev)
    assert done and done[0]["data"] == sets[0] and done[0]["lr_schedule"] == "cosine" and "lr" not in done[0]
    assert done[0]["val_loss"] == ev[1]["val_loss"]
    os.makedirs(tmp_path / "ck2")
    shutil.copy(tmp_path / "ck" / "ckpt-00000002.pt", tmp_path / "ck2")
    ev2, done2 = _launch(common + ["--ckpt-dir", str(tmp_path / "ck2")], 36540)
    assert ev2 == [ev[1]] and done2[0]["steps"] == 2 and done2[0]["final_step"] == 4, (ev, ev2)
