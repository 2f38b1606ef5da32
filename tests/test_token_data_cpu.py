"""Token files on the CPU: the window sampler's host reference, the numpy batch path,
resume, the learning-rate schedule, held-out evaluation, and pdo-launch end to end.

The sampler is defined in paddle_operator_amd/data.py; tests/test_token_data_gpu.py
holds the kernel against this reference.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from paddle_operator_amd import data as D
from paddle_operator_amd.models.gpt2 import GPT2Config
from paddle_operator_amd.ops.core import philox4x32_10
from paddle_operator_amd.ops.optim import cosine_lr
from paddle_operator_amd.train import GPT2Trainer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234_5678_9ABC_DEF1


def _python_starts(seed, stream, m, rank, B, n, S):
    """The definition in Python integers, one Philox call per row."""
    out = []
    for j in range(B):
        w = philox4x32_10((rank * B + j, 0, stream, m & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))
        out.append(((int(w[1]) << 32) | int(w[0])) % (n - S))
    return out


# ----------------------------------------------------------------------------- window_starts
@pytest.mark.parametrize("n,S", [(4099, 128), (130, 128), (2**33 + 7, 1024), (70000, 1)])
def test_window_starts_definition_and_range(n, S):
    for stream in (0, 1):
        for m in (0, 1, 77, 2**32 + 5):
            s = D.window_starts(SEED, stream, m, 3, 8, n, S)
            assert s.dtype == np.int64 and s.shape == (8,)
            assert s.min() >= 0 and s.max() <= n - S - 1
            assert s.tolist() == _python_starts(SEED, stream, m, 3, 8, n, S)


def test_window_starts_single_window_is_zero():
    assert D.window_starts(SEED, 0, 5, 0, 16, 129, 128).tolist() == [0] * 16


def test_window_starts_64bit_modulo():
    """n − S above 2³²: the modulo takes both words (a start beyond 2³² occurs)."""
    n, S = 2**33 + 7, 1024
    s = np.concatenate([D.window_starts(SEED, 0, m, 0, 64, n, S) for m in range(4)])
    assert s.max() >= 2**32
    assert s[:64].tolist() == _python_starts(SEED, 0, 0, 0, 64, n, S)


def test_global_batch_independent_of_split():
    a = np.concatenate([D.window_starts(SEED, 0, 9, r, 4, 4099, 64) for r in range(2)])
    assert a.tolist() == D.window_starts(SEED, 0, 9, 0, 8, 4099, 64).tolist()


def test_streams_steps_and_seeds_differ():
    base = D.window_starts(SEED, 0, 9, 0, 8, 10**6, 64).tolist()
    assert base != D.window_starts(SEED, 1, 9, 0, 8, 10**6, 64).tolist()
    assert base != D.window_starts(SEED, 0, 10, 0, 8, 10**6, 64).tolist()
    assert base != D.window_starts(SEED + (1 << 32), 0, 9, 0, 8, 10**6, 64).tolist()  # the high seed word counts
    assert base == D.window_starts(SEED, 0, 9 + 2**32, 0, 8, 10**6, 64).tolist()  # m mod 2^32


def test_window_starts_rejects_bad_arguments():
    with pytest.raises(ValueError):
        D.window_starts(SEED, 0, 0, 0, 4, 64, 64)  # n < S + 1
    with pytest.raises(ValueError):
        D.window_starts(SEED, 0, 0, 2**30, 8, 4099, 64)  # g ≥ 2^32


# ----------------------------------------------------------------------------- file format, CPU batches
def _write(path, arr):
    np.asarray(arr, dtype="<u2").tofile(path)
    return str(path)


def test_file_format_checks(tmp_path):
    p = _write(tmp_path / "t.bin", np.arange(100) % 50)
    with pytest.raises(ValueError, match="vocab_size"):
        D.open_tokens(p, 16, 65537)
    with pytest.raises(ValueError, match="at least"):
        D.open_tokens(p, 100, 1000)
    assert D.open_tokens(p, 99, 1000).shape == (100,)
    odd = tmp_path / "odd.bin"
    odd.write_bytes(b"\x01" * 201)
    with pytest.raises(ValueError, match="whole number"):
        D.open_tokens(str(odd), 16, 1000)


def test_cpu_batch_is_the_window_gather(tmp_path):
    rng = np.random.default_rng(0)
    corpus = rng.integers(0, 1000, 4099)
    p = _write(tmp_path / "t.bin", corpus)
    ts = D.TokenStream(p, 5, 127, 1000, "cpu", seed=SEED, rank=2)
    for m in (0, 3):
        idx, tgt = ts.batch(m)
        starts = D.window_starts(SEED, 0, m, 2, 5, 4099, 127)
        assert idx.dtype == tgt.dtype == torch.int64 and idx.shape == tgt.shape == (5, 127)
        for r, s in enumerate(starts):
            assert idx[r].tolist() == corpus[s:s + 127].tolist()
            assert tgt[r].tolist() == corpus[s + 1:s + 128].tolist()


def test_out_of_vocab_ids_are_masked_counted_and_raise(tmp_path):
    corpus = np.arange(300) % 100
    corpus[::7] = 1000  # id = vocab
    p = _write(tmp_path / "t.bin", corpus)
    ts = D.TokenStream(p, 2, 32, 1000, "cpu", seed=1)
    idx, tgt, bad = ts.host_batch(0)
    w = ts.windows(0).astype(np.int64)
    assert bad == int((w >= 1000).sum()) > 0
    assert torch.equal(idx, torch.from_numpy(np.where(w >= 1000, 0, w)[:, :-1]))
    assert torch.equal(tgt, torch.from_numpy(np.where(w >= 1000, -1, w)[:, 1:]))
    tr = GPT2Trainer(GPT2Config.named("gpt2-tiny"), 2, 32, "cpu", dtype=torch.float32, data=p, data_seed=1)
    with pytest.raises(ValueError, match=r"t\.bin.*token id"):
        tr.step()


# ----------------------------------------------------------------------------- trainer: resume, schedule, evaluation
@pytest.fixture(scope="module")
def corpus_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    rng = np.random.default_rng(5)
    return _write(d / "train.bin", rng.integers(0, 1000, 6000)), _write(d / "val.bin", rng.integers(0, 1000, 3000))


def _trainer(files, **kw):
    return GPT2Trainer(GPT2Config.named("gpt2-tiny"), 2, 32, "cpu", dtype=torch.float32, data=files[0],
                       val_data=files[1], data_seed=11, **kw)


def _run(tr, steps):
    """(loss, the step's token batches) per step."""
    seen, out = [], []
    batch = tr.batch

    def spy():
        x, y = batch()
        seen.append((x.clone(), y.clone()))
        return x, y
    tr.batch = spy
    for _ in range(steps):
        n0 = len(seen)
        loss = float(tr.step().detach())
        out.append((loss, seen[n0:]))
    tr.batch = batch
    return out


@pytest.mark.parametrize("K", [1, 2])
def test_resume_replays_batches_and_losses(corpus_files, K):
    straight = _run(_trainer(corpus_files, grad_accum=K), 4)
    a = _trainer(corpus_files, grad_accum=K)
    first = _run(a, 2)
    st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    st["opt"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st["opt"].items()}
    assert st["data_step"] == 2 * K
    b = _trainer(corpus_files, grad_accum=K)
    b.load_state_dict(st, 2)
    resumed = first + _run(b, 2)
    for (l0, b0), (l1, b1) in zip(straight, resumed):
        assert l0 == l1
        assert len(b0) == len(b1) == K
        for (x0, y0), (x1, y1) in zip(b0, b1):
            assert torch.equal(x0, x1) and torch.equal(y0, y1)
    assert not torch.equal(straight[0][1][0][0], straight[1][1][0][0])  # the stream moves
    # a checkpoint from before data_step: the stream resumes at step · K
    del st["data_step"]
    c = _trainer(corpus_files, grad_accum=K)
    c.load_state_dict(st, 2)
    assert c.data_step == 2 * K


def test_lr_schedule_passed_to_the_optimizer(corpus_files):
    def rates(tr, n):
        got, step = [], tr.opt.step

        def spy(grad_scale=1.0, lr=None):
            got.append(tr.opt.lr if lr is None else lr)
            return step(grad_scale=grad_scale, lr=lr)
        tr.opt.step = spy
        for _ in range(n):
            tr.step()
        return got

    kw = dict(lr=1e-3, lr_warmup=2, lr_decay_steps=5, lr_min_ratio=0.2)
    want = [cosine_lr(s, 1e-3, 2, 5, 0.2) for s in range(7)]
    assert rates(_trainer(corpus_files, lr_schedule="cosine", **kw), 7) == want
    assert want[0] == 5e-4 and want[2] == 1e-3 and math.isclose(want[6], 2e-4)
    assert rates(_trainer(corpus_files, lr_schedule="cosine", grad_accum=2, **kw), 3) == want[:3]  # per optimizer step
    assert rates(_trainer(corpus_files), 3) == [3e-4] * 3
    # step_count is in the checkpoint: a resumed job continues the curve
    a = _trainer(corpus_files, lr_schedule="cosine", **kw)
    rates(a, 3)
    b = _trainer(corpus_files, lr_schedule="cosine", **kw)
    b.load_state_dict(a.state_dict(), 3)
    assert rates(b, 2) == want[3:5]


def test_evaluate_is_repeatable_and_leaves_training_untouched(corpus_files):
    a, b = _trainer(corpus_files), _trainer(corpus_files)
    a.step()
    b.step()
    counters = (a.drop_step, a.data_step, a.opt.step_count)
    grads = a.flat.grads.clone()
    v0 = a.evaluate(3)
    assert v0 == a.evaluate(3) and math.isfinite(v0)
    assert a.model.training and (a.drop_step, a.data_step, a.opt.step_count) == counters
    assert torch.equal(a.flat.grads, grads)
    # the evaluation windows are those of stream 1 of val.bin, m = 0 … 2
    want = D.TokenStream(corpus_files[1], 2, 32, 1000, "cpu", seed=11, stream=1)
    a.model.eval()
    with torch.no_grad():
        ref = np.mean([float(a.model(*want.batch(m))) for m in range(3)])
    a.model.train()
    assert abs(v0 - ref) < 1e-5
    a.step()
    b.step()
    assert torch.equal(a.flat.params, b.flat.params) and torch.equal(a.opt.master, b.opt.master)
    with pytest.raises(RuntimeError):
        GPT2Trainer(GPT2Config.named("gpt2-tiny"), 2, 32, "cpu", dtype=torch.float32).evaluate(1)


def test_accumulation_matches_one_large_batch_in_fp32():
    """K = 3 micro-batches of 2 rows against one batch of 6 (fp32 on the CPU: only
    summation order differs), through the init / emit sequence of the fp32 accumulator."""
    cfg = GPT2Config.named("gpt2-tiny")
    big = GPT2Trainer(cfg, 6, 32, "cpu", dtype=torch.float32)
    acc = GPT2Trainer(cfg, 2, 32, "cpu", dtype=torch.float32, grad_accum=3)
    assert acc.acc is not None and GPT2Trainer(cfg, 2, 32, "cpu", dtype=torch.float32, grad_accum=2).acc is None
    x, y = big.batch()
    lb, la = float(big.step(x, y).detach()), float(acc.step(x, y).detach())
    assert abs(lb - la) < 1e-5
    assert (big.flat.grads - acc.flat.grads).norm() <= 1e-5 * big.flat.grads.norm()
    assert acc.drop_step == acc.data_step == 3 and acc.opt.step_count == 1 and acc.tokens_per_step() == 3 * 2 * 32
    with pytest.raises(ValueError):
        acc.step(x[:4], y[:4])


# ----------------------------------------------------------------------------- pdo-launch end to end
def _launch(args, log, env_extra=None):
    env = dict(os.environ)
    env.update({"OMP_NUM_THREADS": "2", "PYTHONPATH": REPO, "PDO_OPS": "torch", "CUDA_VISIBLE_DEVICES": "",
                "HIP_VISIBLE_DEVICES": ""})
    env.pop("PDO_TRAIN_DATA", None)
    env.pop("PDO_VAL_DATA", None)
    env.update(env_extra or {})
    with open(log, "w") as f:
        rc = subprocess.run([sys.executable, "-m", "paddle_operator_amd.launch"] + args, env=env, cwd=REPO, stdout=f,
                            stderr=subprocess.STDOUT, timeout=240).returncode
    text = open(log).read()
    assert rc == 0, text[-3000:]
    recs = {}
    for line in text.splitlines():
        tag, _, rest = line.partition(" ")
        if tag in ("PDO_DONE", "PDO_EVAL"):
            recs.setdefault(tag, []).append(json.loads(rest))
    return recs


def _markov_corpus(n, seed):
    """64 symbols; x' = (5x + 17) mod 64 with probability 0.9, else uniform."""
    rng = np.random.default_rng(seed)
    jump, unif = rng.random(n) < 0.9, rng.integers(0, 64, n)
    x = np.empty(n, dtype=np.int64)
    x[0] = unif[0]
    for i in range(1, n):
        x[i] = (5 * x[i - 1] + 17) % 64 if jump[i] else unif[i]
    return x


def test_launch_trains_on_token_files(tmp_path):
    corpus = _markov_corpus(200_000, 0)
    train = _write(tmp_path / "train.bin", corpus)
    val = _write(tmp_path / "val.bin", _markov_corpus(20_000, 1))
    counts = np.bincount(corpus, minlength=64).astype(np.float64)
    p = counts / counts.sum()
    unigram = float(-(p[p > 0] * np.log(p[p > 0])).sum())
    assert 4.1 < unigram <= math.log(64)
    recs = _launch(["--workload", "gpt2", "--tiny", "--batch", "4", "--seq", "64", "--steps", "200", "--log-every", "50",
                    "--val-data", val, "--eval-every", "100", "--eval-batches", "4"], tmp_path / "run.log",
                   {"PDO_TRAIN_DATA": train})  # the environment default of --data
    evals, done = recs["PDO_EVAL"], recs["PDO_DONE"][0]
    assert [e["step"] for e in evals] == [100, 200]
    final = evals[-1]["val_loss"]
    print(f"unigram entropy {unigram:.4f}; val_loss {[round(e['val_loss'], 4) for e in evals]}")
    assert final < unigram and final < evals[0]["val_loss"]
    assert done["val_loss"] == final and done["data"] == train and done["steps"] == 200
    assert "grad_accum" not in done and "lr_schedule" not in done


def test_launch_flags_reach_the_records(tmp_path):
    train = _write(tmp_path / "train.bin", _markov_corpus(5000, 2))
    done = _launch(["--workload", "gpt2", "--tiny", "--batch", "2", "--seq", "32", "--steps", "3", "--data", train,
                    "--grad-accum", "2", "--lr-schedule", "cosine", "--lr-warmup", "1"], tmp_path / "run.log")["PDO_DONE"][0]
    assert done["grad_accum"] == 2 and done["lr_schedule"] == "cosine" and done["data"] == train
    assert "val_loss" not in done
    assert math.isclose(done["throughput"] * done["seconds"], 3 * 2 * 2 * 32)  # K micro-batches per step


def test_eval_every_needs_val_data(monkeypatch):
    from paddle_operator_amd.launch.run import parse_args
    monkeypatch.delenv("PDO_VAL_DATA", raising=False)
    with pytest.raises(SystemExit):
        parse_args(["--workload", "gpt2", "--eval-every", "10"])
    a = parse_args(["--workload", "gpt2", "--eval-every", "10", "--val-data", "v.bin"])
    assert a.val_data == "v.bin" and a.grad_accum is None and a.lr_schedule is None and a.lr == 3e-4


def test_bench_record_carries_the_given_flags(tmp_path):
    train = _write(tmp_path / "train.bin", _markov_corpus(5000, 2))
    base = ["--workload", "gpt2", "--tiny", "--batch", "2", "--seq", "32", "--steps", "2", "--warmup", "1", "--bench"]
    for extra, keys in ((["--data", train, "--grad-accum", "3"], {"data", "grad_accum"}), ([], set())):
        env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=REPO, PDO_OPS="torch", HIP_VISIBLE_DEVICES="",
                   CUDA_VISIBLE_DEVICES="")
        env.pop("PDO_TRAIN_DATA", None)
        r = subprocess.run([sys.executable, "-m", "paddle_operator_amd.launch"] + base + extra, env=env, cwd=REPO,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        rec = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("PDO_BENCH "))[len("PDO_BENCH "):])
        assert {"data", "grad_accum", "lr_schedule", "val_loss"} & set(rec) == keys
        assert rec["tokens_per_step_rank"] == 2 * 32 * (3 if extra else 1)


def test_two_ranks_see_the_global_batch_of_one(tmp_path):
    """World 2 × B 2 trains and evaluates on the rows of world 1 × B 4: the same global
    batches.  fp32 on the CPU, so only the order of the gradient mean differs (two half-batch
    means averaged by the all-reduce against one mean), which four Adam steps amplify a
    little; other training rows move this val_loss by about 1e-2 relative (the same corpus
    rotated by 1000 tokens: 6.37 → 6.28), so 1e-4 relative separates the two."""
    import random
    import socket
    train = _write(tmp_path / "train.bin", _markov_corpus(20_000, 3))
    val = _write(tmp_path / "val.bin", _markov_corpus(5_000, 4))
    args = ["--workload", "gpt2", "--tiny", "--seq", "32", "--steps", "4", "--data", train, "--val-data", val,
            "--eval-every", "4", "--eval-batches", "2", "--data-seed", "3"]
    one = _launch(args + ["--batch", "4"], tmp_path / "one.log")["PDO_EVAL"][0]["val_loss"]
    rng = random.Random(os.getpid())
    for _ in range(50):  # a base port whose rendezvous ports are free (launch/env.py derives them)
        base = rng.randrange(12000, 31000)
        try:
            for q in range(base, base + 40):
                s = socket.socket()
                s.bind(("127.0.0.1", q))
                s.close()
            break
        except OSError:
            continue
    eps = ",".join(f"127.0.0.1:{base + 20 * i}" for i in range(2))
    procs, logs = [], []
    for r in range(2):
        env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=REPO, PDO_OPS="torch", HIP_VISIBLE_DEVICES="",
                   CUDA_VISIBLE_DEVICES="", PADDLE_TRAINER_ID=str(r), PADDLE_TRAINER_ENDPOINTS=eps,
                   PADDLE_TRAINERS_NUM="2", POD_IP="127.0.0.1", PADDLE_PORT=str(base + 20 * r), TRAINING_ROLE="TRAINER")
        logs.append(open(tmp_path / f"r{r}.log", "w"))
        procs.append(subprocess.Popen([sys.executable, "-m", "paddle_operator_amd.launch"] + args + ["--batch", "2"],
                                      env=env, cwd=REPO, stdout=logs[-1], stderr=subprocess.STDOUT))
    try:
        assert [p.wait(240) for p in procs] == [0, 0], open(tmp_path / "r0.log").read()[-3000:]
    finally:
        for p, f in zip(procs, logs):
            if p.poll() is None:
                p.kill()
            f.close()
    text = open(tmp_path / "r0.log").read()
    two = json.loads(next(ln for ln in text.splitlines() if ln.startswith("PDO_EVAL "))[len("PDO_EVAL "):])["val_loss"]
    assert "PDO_EVAL" not in open(tmp_path / "r1.log").read()  # rank 0 reports
    print(f"val_loss after 4 steps: world 1 × B 4 {one:.6f}, world 2 × B 2 {two:.6f}")
    assert abs(one - two) < 1e-4 * one


def test_launch_without_the_new_flags_keeps_its_record(tmp_path):
    done = _launch(["--workload", "gpt2", "--tiny", "--seq", "32", "--steps", "2"], tmp_path / "run.log")["PDO_DONE"][0]
    assert sorted(done) == sorted(["rank", "world", "steps", "seconds", "throughput", "final_step", "ready_s",
                                   "dropout", "attn_dropout"])
