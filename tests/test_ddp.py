"""Data-parallel correctness on CPU (gloo, 2 ranks) and the bench.py contract.

* BucketedDDP (parallel/ddp.py): two ranks on half batches, small buckets so
  the backward issues many bucket all-reduces out of autograd order — the
  averaged arena gradients must equal a single process's full-batch
  gradients.  Same code path as RCCL on 8×MI355X, only the backend differs.
* bench.py: the driver's contract (one JSON line, whole-job value, n_gpus =
  world size) for N=1 and for N=2 under torch.distributed.run.
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batch(cfg, B=4, S=32):
    g = torch.Generator().manual_seed(7)
    idx = torch.randint(0, cfg.vocab_size, (B, S + 1), generator=g)
    return idx[:, :-1], idx[:, 1:]


def _ddp_worker(rank, world, port, outdir, split=()):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PDO_OPS="torch")
    torch.set_num_threads(2)
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    from paddle_operator_amd.parallel.ddp import BucketedDDP
    from paddle_operator_amd.parallel.flat import FlatParams

    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = GPT2Config.named("gpt2-tiny")
    model = GPT2(cfg)
    flat = FlatParams(model, dtype=torch.float32, device="cpu", bucket_bytes=64 << 10, late=("wte",), split=split)
    ddp = BucketedDDP(flat)
    assert len(flat.buckets) > 4  # many buckets → out-of-order readiness is exercised
    if split:  # the LM-head half of the tied weight is bucket 0, the embedding half the last
        assert [s.name for s in flat.buckets[0].slots] == ["wte#head"]
        assert "wte" in [s.name for s in flat.buckets[-1].slots]
        launched = []
        orig = ddp._launch
        ddp._launch = lambda i: (launched.append((i, len(ddp._seen))), orig(i))[1]
    x, y = _batch(cfg)
    per = x.shape[0] // world
    sl = slice(rank * per, (rank + 1) * per)
    for _ in range(2):  # second step: bookkeeping reset by prepare()
        flat.zero_grad()
        ddp.prepare()
        model(x[sl], y[sl]).backward()
        ddp.finish()
        if split:
            # bucket 0 went out after the first gradient of the backward (the head's),
            # long before the last bucket; the slot is folded and zeroed afterwards
            assert launched[0] == (0, 1), launched
            assert float(flat.aux_slots[0].param.grad.abs().max()) == 0.0
            launched.clear()
    torch.save({n: (p.grad * ddp.grad_scale).clone() for n, p in model.named_parameters()},
               os.path.join(outdir, f"g{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("split", [(), ("wte",)])
def test_bucketed_ddp_matches_full_batch(tmp_path, split):
    """split = ("wte",): the tied weight's LM-head gradient in its own first
    bucket (parallel/flat.py AuxGrad), folded after the drain — same gradients."""
    os.environ["PDO_OPS"] = "torch"
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config

    mp.start_processes(_ddp_worker, args=(2, _free_port(), str(tmp_path), split), nprocs=2, start_method="spawn")
    cfg = GPT2Config.named("gpt2-tiny")
    ref = GPT2(cfg)  # same deterministic init as the ranks
    x, y = _batch(cfg)
    ref(x, y).backward()
    g0 = torch.load(tmp_path / "g0.pt", weights_only=True)
    g1 = torch.load(tmp_path / "g1.pt", weights_only=True)
    for n, p in ref.named_parameters():
        assert torch.equal(g0[n], g1[n]), f"ranks disagree on {n}"
        err = (g0[n] - p.grad).norm() / (p.grad.norm() + 1e-12)
        assert err < 1e-5, f"{n}: rel err {err}"


def _norm_order_worker(rank, world, port, outdir, early):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PDO_OPS="torch")
    torch.set_num_threads(1)
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    from paddle_operator_amd.ops.optim import FlatAdamW
    from paddle_operator_amd.parallel.ddp import BucketedDDP
    from paddle_operator_amd.parallel.flat import FlatParams

    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = GPT2Config.named("gpt2-tiny")
    model = GPT2(cfg)
    flat = FlatParams(model, dtype=torch.float32, device="cpu", bucket_bytes=64 << 10, late=("wte",), split=("wte",))
    ddp = BucketedDDP(flat)
    # a small clip so the coefficient is active; small chunks so buckets own many of them
    opt = FlatAdamW(flat, lr=1e-3, max_grad_norm=0.05, norm_chunk=4096)
    x, y = _batch(cfg, B=8)
    per = x.shape[0] // world
    sl = slice(rank * per, (rank + 1) * per)
    early_chunks = []
    for _ in range(3):
        flat.zero_grad()
        ddp.prepare()
        model(x[sl], y[sl]).backward()
        ddp.finish(opt if early else None)
        early_chunks.append(opt._norm_next)
        opt.step(grad_scale=ddp.grad_scale)
    torch.save({"params": flat.params.clone(), "early_chunks": early_chunks, "nchunks": opt._norm_part.numel(),
                "fold_chunk": ddp._fold_start // 4096}, os.path.join(outdir, f"p{rank}_{int(early)}.pt"))
    dist.destroy_process_group()


def test_norm_partials_per_bucket_bit_identical(tmp_path):
    """BucketedDDP.finish(opt) sums each parameter bucket's global-norm chunks as
    its all-reduce lands (only the tied embedding's tail range waits for the
    step): 4 ranks, 3 clipped AdamW steps, parameters bit-identical to
    finish() followed by the whole-range norm in the step."""
    os.environ["PDO_OPS"] = "torch"
    for early in (False, True):
        mp.start_processes(_norm_order_worker, args=(4, _free_port(), str(tmp_path), early), nprocs=4,
                           start_method="spawn")
    for r in range(4):
        a = torch.load(tmp_path / f"p{r}_0.pt", weights_only=True)
        b = torch.load(tmp_path / f"p{r}_1.pt", weights_only=True)
        assert torch.equal(a["params"], b["params"]), f"rank {r}: parameters differ"
        assert a["early_chunks"] == [0, 0, 0]
        # everything before the tied embedding's slot was summed before the step
        assert all(c == b["fold_chunk"] for c in b["early_chunks"]), (b["early_chunks"], b["fold_chunk"])
        assert 0 < b["fold_chunk"] < b["nchunks"]
    a0 = torch.load(tmp_path / "p0_1.pt", weights_only=True)["params"]
    for r in range(1, 4):
        assert torch.equal(a0, torch.load(tmp_path / f"p{r}_1.pt", weights_only=True)["params"])


def _bench_env():
    env = dict(os.environ, PYTHONPATH=REPO, OMP_NUM_THREADS="2", PDO_OPS="torch")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


BENCH_ARGS = ["--model", "gpt2-tiny", "--micro-batch", "2", "--seq", "64", "--steps", "2", "--warmup", "1",
              "--ready-trials", "2", "--cpu", "--ops", "torch", "--compat-trials", "1", "--train-ready-trials", "2",
              "--b2b-trials", "2", "--full"]


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _check_record(rec, n):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "ready_p50_s"):
        assert k in rec, k
    assert rec["n_gpus"] == n and rec["steps"] == 2 and rec["warmup"] == 1 and rec["value"] > 0
    assert rec["config"]["parallelism"] == f"dp{n}" and rec["config"]["global_batch"] == 2 * n
    assert "PaddleJob" in rec["config"]["launch"] and rec["config"]["pod_layout"] in (f"{n}x1", f"1x{n}")
    assert rec["ready"]["trials"] == 2 and 0 < rec["ready_p50_s"] < 60
    assert rec["ready_train"]["trials"] == 2 and rec["ready_b2b"]["trials"] == 2
    assert rec["compat_ready"]["trials"] == 1 and rec["compat_ready"]["p50"] > 0
    if n > 1:  # communication evidence measured after the timed region (launch/run.py _comm_diag)
        c = rec["comm"]
        assert c["ranks"] == n and c["allreduce_busbw_GBps_min"] > 0 and "exposed_ms_max" in c, c
        sw = c["allreduce_sweep"]
        assert [p["bytes"] >> 20 for p in sw] == [1, 2, 4, 8] and all(p["busbw_GBps"] > 0 for p in sw), sw
        assert c["knee_bytes"] in [p["bytes"] for p in sw]
        assert c["buckets"]["count"] >= 1 and all(b > 0 for b in c["buckets"]["bytes"])
    else:
        assert rec["comm"] is None
    tokens = 2 * 64 * n * 2  # micro-batch × seq × world × steps
    assert abs(rec["value"] - tokens / (rec["ms_per_step"] * 2 / 1e3)) / rec["value"] < 1e-2


def test_bench_launched_single():
    """bench.py launches a 1-rank PaddleJob through the operator (no torchrun)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + BENCH_ARGS, cwd=REPO, env=_bench_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_record(_json_line(r.stdout), 1)


def test_bench_launched_two_ranks_without_torchrun():
    """--gpus 2 spawns both ranks itself (agent fork/exec via the warm launcher)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + BENCH_ARGS, cwd=REPO, env=_bench_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_record(_json_line(r.stdout), 2)


def test_bench_one_pod_layout_two_ranks():
    """--pod-layout one-pod: one PaddleJob pod running --nproc-per-pod 2 local
    ranks (the Kubernetes xGMI layout); the record says which layout ran."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--pod-layout", "one-pod"] + BENCH_ARGS, cwd=REPO,
                       env=_bench_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    _check_record(rec, 2)
    assert rec["config"]["pod_layout"] == "1x2" and "replicas=1 x 2" in rec["config"]["launch"]


@pytest.mark.parametrize("layout", ["per-gpu", "one-pod"])
def test_bench_eight_ranks_virtual_gpus(layout):
    """The 8-GPU launched path on CPU: the node offers 8 (virtual) GPUs, so the
    agent's GPU accounting, the warm launcher's one-slot-per-GPU pool (above 2
    GPUs) and the 8-rank comm block all run as on a full MI355X node; the ranks
    themselves train the tiny ResNet over gloo.  Both pod layouts: 8 × 1 GPU and
    1 × 8 GPUs (--nproc-per-pod 8)."""
    env = _bench_env()
    env.pop("PDO_SLOTS_PER_GPU", None)
    args = ["--gpus", "8", "--cpu", "--virtual-gpus", "--workload", "resnet50", "--tiny", "--micro-batch", "2",
            "--steps", "2", "--warmup", "1", "--ready-trials", "2", "--compat-trials", "0", "--train-ready-trials", "1",
            "--b2b-trials", "1", "--ops", "torch", "--pod-layout", layout, "--full"]
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    assert rec["n_gpus"] == 8 and rec["config"]["parallelism"] == "dp8" and rec["config"]["global_batch"] == 16
    assert rec["config"]["pod_layout"] == ("8x1" if layout == "per-gpu" else "1x8")
    slots = rec["warm_slots"]["node0"]
    assert sorted(slots, key=int) == [str(i) for i in range(8)]
    assert all(sl["n"] == 1 for sl in slots.values()), slots  # one warm slot per GPU above 2 GPUs
    c = rec["comm"]
    assert c["ranks"] == 8 and c["buckets"]["count"] >= 1 and len(c["allreduce_sweep"]) == 4
    assert c["nosync_step_ms_max"] < 5000  # forked ranks honour the pod's OMP_NUM_THREADS
    assert rec["ready"]["trials"] == 2 and rec["ready_b2b"]["trials"] == 1


def test_bench_eight_virtual_gpus_gang_and_secondary():
    """Configs 3 and 4 in the 8-GPU driver run, rehearsed on CPU: the GPT-2 job
    goes through the Volcano gang path (PodGroup minMember=8, admitted before any
    pod binds, Running once all 8 run — reference controllers/paddlejob_helper.go
    :478-549), the ResNet job (deploy/examples/resnet.yaml) runs on the same 8
    ranks under 'secondary', and both records carry the comm block."""
    env = _bench_env()
    env.pop("PDO_SLOTS_PER_GPU", None)
    args = ["--gpus", "8", "--cpu", "--virtual-gpus", "--model", "gpt2-tiny", "--micro-batch", "2", "--seq", "64",
            "--steps", "2", "--warmup", "1", "--ready-trials", "1", "--compat-trials", "0", "--train-ready-trials", "0",
            "--b2b-trials", "0", "--ops", "torch", "--full"]
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    assert rec["n_gpus"] == 8 and rec["config"]["parallelism"] == "dp8"
    g = rec["gang"]
    assert g["podgroup_min_member"] == 8 and g["bound_before_inqueue"] == 0, g
    assert g["podgroup_phases"][-1] == "Running" and "Inqueue" in g["podgroup_phases"] + ["Inqueue"], g
    assert g["bound_pods"] == 8, g
    assert "gang=volcano PodGroup minMember=8" in rec["config"]["launch"]
    c = rec["comm"]
    assert c["ranks"] == 8 and c["buckets"]["count"] >= 1 and c["allreduce_busbw_GBps_min"] > 0, c
    sec = rec["secondary"]
    assert "error" not in sec, sec
    assert sec["n_gpus"] == 8 and sec["value"] > 0 and sec["config"]["parallelism"] == "dp8"
    assert sec["gang"]["podgroup_min_member"] == 8 and sec["gang"]["bound_before_inqueue"] == 0
    assert sec["comm"]["ranks"] == 8


@pytest.mark.slow
def test_bench_contract_torchrun_two_ranks():
    """Under the driver's torchrun wrapper: rank 0 launches, rank 1 only waits; one JSON line."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2"] + BENCH_ARGS
    r = subprocess.run(cmd, cwd=REPO, env=_bench_env(), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    _check_record(_json_line(r.stdout), 2)


def test_bucket_policy():
    from paddle_operator_amd.utils.topology import bucket_bytes_for
    MiB = 1 << 20
    gpt2m = 355 * 10**6 * 2  # bf16 gradient bytes
    assert bucket_bytes_for(1, gpt2m) == gpt2m  # nothing to overlap with at world 1
    assert bucket_bytes_for(8, gpt2m) == 56 * MiB  # 8 ranks × 7 links × 1 MiB
    assert bucket_bytes_for(2, gpt2m) == 16 * MiB  # floor
    assert bucket_bytes_for(8, 100 * MiB) == 25 * MiB  # ≥ 4 buckets for small models
    assert bucket_bytes_for(64, 10**12) == 256 * MiB  # cap


def _prec_worker(rank, world, port, outdir, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PDO_OPS="torch")
    torch.set_num_threads(1)
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    from paddle_operator_amd.parallel.ddp import BucketedDDP
    from paddle_operator_amd.parallel.flat import FlatParams

    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = GPT2Config.named("gpt2-tiny")
    model = GPT2(cfg).to(torch.bfloat16)
    flat = FlatParams(model, dtype=torch.bfloat16, device="cpu", bucket_bytes=64 << 10, late=("wte",))
    ddp = BucketedDDP(flat, grad_reduce=mode)
    x, y = _batch(cfg, B=8)
    per = x.shape[0] // world
    sl = slice(rank * per, (rank + 1) * per)
    flat.zero_grad()
    ddp.prepare()
    model(x[sl], y[sl]).backward()
    ddp.finish()
    if rank == 0:
        torch.save((flat.grads.float() * ddp.grad_scale).clone(), os.path.join(outdir, f"{mode}.pt"))
    dist.destroy_process_group()


def test_grad_reduce_precision_4_ranks(tmp_path):
    """bf16 vs fp32 gradient reduction at 4 ranks against the fp32 full-batch gradient.

    Pins the claim in parallel/ddp.py: summing bf16 buckets on the wire adds
    little to the error the bf16 model already has — the bf16-wire DDP
    gradient stays within 1.5× of one process's full-batch bf16 gradient error,
    and the fp32 wire is no worse than that either."""
    os.environ["PDO_OPS"] = "torch"
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    from paddle_operator_amd.parallel.flat import FlatParams

    for mode in ("bf16", "fp32"):
        mp.start_processes(_prec_worker, args=(4, _free_port(), str(tmp_path), mode), nprocs=4,
                           start_method="spawn")
    cfg = GPT2Config.named("gpt2-tiny")
    x, y = _batch(cfg, B=8)

    def full_batch(dtype):
        m = GPT2(cfg).to(dtype)
        f = FlatParams(m, dtype=dtype, device="cpu", bucket_bytes=64 << 10, late=("wte",))
        f.zero_grad()
        m(x, y).backward()
        return f.grads.float().clone()

    ref = full_batch(torch.float32)
    single = full_batch(torch.bfloat16)

    def rel(g):
        return float((g - ref).norm() / ref.norm())

    e_single = rel(single)
    e_bf16 = rel(torch.load(tmp_path / "bf16.pt", weights_only=True))
    e_fp32 = rel(torch.load(tmp_path / "fp32.pt", weights_only=True))
    assert e_single < 0.05, e_single  # sanity: the bf16 model itself
    assert e_bf16 < 1.5 * e_single + 1e-3, (e_bf16, e_single)
    assert e_fp32 < 1.5 * e_single + 1e-3, (e_fp32, e_single)


def _bcast_worker(rank, world, port, q):
    import torch.distributed as dist
    from paddle_operator_amd.parallel.ddp import broadcast_buffers
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    ts = [torch.full((3, 2), float(rank)), torch.full((5,), float(rank) + 0.5), torch.tensor(rank, dtype=torch.long)]
    broadcast_buffers(ts, 0)
    q.put((rank, [t.tolist() for t in ts]))
    dist.destroy_process_group()


def test_broadcast_buffers_one_collective_per_dtype():
    """ResNet BN running stats + counters reach every rank from rank 0."""
    import torch.multiprocessing as mp
    from test_launch import free_port_block
    port = free_port_block(2)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_bcast_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in ps:
        p.start()
    out = dict(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(60)
    for r in range(3):
        assert out[r] == [[[0.0, 0.0]] * 3, [0.5] * 5, 0], out[r]


def test_bench_launched_resnet_workload():
    """bench.py --workload resnet50 (configs 2/3 through the operator): images/s record."""
    args = ["--workload", "resnet50", "--tiny", "--micro-batch", "4", "--steps", "2", "--warmup", "1",
            "--ready-trials", "1", "--cpu", "--full"]
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + args, cwd=REPO, env=_bench_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    assert rec["unit"] == "images/s" and rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 8
    assert abs(rec["value"] - 4 * 2 * 2 / (rec["ms_per_step"] * 2 / 1e3)) / rec["value"] < 1e-2


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """Without --full only the throughput job runs (the trial flags are ignored,
    their fields null); --steps sets the timed steps; --dump-outputs writes the
    last timed step's loss and its parameter / gradient arenas as float32 .npy."""
    import numpy as np
    out = tmp_path / "dump"
    args = ["--gpus", "1", "--model", "gpt2-tiny", "--micro-batch", "2", "--seq", "64", "--steps", "3", "--warmup", "1",
            "--cpu", "--ops", "torch", "--ready-trials", "2", "--dump-outputs", str(out)]
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=REPO, env=_bench_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "tokens/s" and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 2 * 64 / (rec["ms_per_step"] / 1e3)) / rec["value"] < 1e-2
    for k in ("ready", "ready_p50_s", "ready_train", "ready_b2b", "compat_ready", "warm_slots"):
        assert rec[k] is None, (k, rec[k])
    assert "secondary" not in rec
    arrays = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert sorted(arrays) == ["grads", "loss", "params"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays["loss"].shape == (1,) and float(arrays["loss"][0]) == pytest.approx(rec["final_loss"])
    assert arrays["params"].size > 1000 and arrays["grads"].size >= arrays["params"].size
    assert np.abs(arrays["grads"]).max() > 0


def test_flat_shadow_scope_cpu():
    """FlatParams.enable_shadow: the low-precision copy of the arena is refreshed
    on entering shadow_scope, readable (shadow_live) only inside it, and each
    parameter's _pdo_shadow view aliases its slice with the parameter's strides."""
    import torch

    from paddle_operator_amd.parallel.flat import FlatParams

    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, bias=False), torch.nn.Linear(16, 4))
    m = m.to(memory_format=torch.channels_last)
    flat = FlatParams(m, dtype=torch.float32, device=torch.device("cpu"))
    flat.enable_shadow(torch.bfloat16)
    w = m[0].weight
    arena, view = w._pdo_shadow
    assert arena is flat and not flat.shadow_live
    assert view.shape == w.shape and view.stride() == w.stride() and view.dtype == torch.bfloat16
    with flat.shadow_scope():
        assert flat.shadow_live
        assert torch.equal(view, w.detach().to(torch.bfloat16))
    assert not flat.shadow_live
    with torch.no_grad():
        w.add_(1.0)  # a change outside the scope: the next scope refreshes
    with flat.shadow_scope():
        assert torch.equal(view, w.detach().to(torch.bfloat16))


def _two_forward_worker(rank, world, port, outdir):
    """Two graphs through the split LM head before one backward, DDP on: bucket
    0 (the head slot) must launch only after BOTH nodes added their part."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PDO_OPS="torch")
    torch.set_num_threads(1)
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    from paddle_operator_amd.parallel.ddp import BucketedDDP
    from paddle_operator_amd.parallel.flat import FlatParams

    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    cfg = GPT2Config.named("gpt2-tiny")
    model = GPT2(cfg)
    flat = FlatParams(model, dtype=torch.float32, device="cpu", bucket_bytes=64 << 10, late=("wte",),
                      split=("wte",))
    ddp = BucketedDDP(flat)
    sp = flat.aux_slots[0].param
    seen = []
    if ddp.enabled:
        orig = ddp._launch

        def launch(i):  # the head slot's node count when its bucket goes on the wire
            if i == 0:
                seen.append((sp.nodes, done[0]))
            orig(i)
        ddp._launch = launch
    done = [0]
    orig_done = sp.node_done

    def node_done():
        done[0] += 1
        orig_done()
    sp.node_done = node_done
    x, y = _batch(cfg, B=8)
    per = x.shape[0] // world
    sl = slice(rank * per, (rank + 1) * per)
    flat.zero_grad()
    ddp.prepare()
    loss = model(x[sl], y[sl]) + 0.5 * model(x[sl].flip(1), y[sl].flip(1))
    loss.backward()
    ddp.finish()
    if rank == 0:
        torch.save({"grads": {n: (p.grad.float() * ddp.grad_scale).clone() for n, p in model.named_parameters()},
                    "seen": seen, "done": done[0]}, os.path.join(outdir, f"w{world}.pt"))
    if world > 1:
        dist.destroy_process_group()


def test_split_head_two_forwards_ddp_two_ranks(tmp_path):
    """ADVICE r5 (ops/gpt2.py:552): with two LM-head graphs before one backward,
    bucket 0 (the split head slot) is launched once, after the second node's
    add — and the 2-rank averaged gradients equal one process's full batch."""
    port = _free_port()
    mp.start_processes(_two_forward_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    _two_forward_worker(0, 1, port, str(tmp_path))
    d2 = torch.load(tmp_path / "w2.pt", weights_only=True)
    d1 = torch.load(tmp_path / "w1.pt", weights_only=True)
    assert d2["done"] == 2 and d2["seen"] == [(0, 2)], d2["seen"]
    for n, r in d1["grads"].items():
        err = float((d2["grads"][n] - r).norm() / (r.norm() + 1e-12))
        assert err < 1e-4, (n, err)


def test_legacy_checkpoint_layout_loads():
    """ADVICE r5 (flat.py:309): an arena checkpoint from before the split head
    slot moved behind the parameter range (params / master / m / v led by the
    aligned wte-sized slot) still loads; another model's buffer still raises."""
    os.environ["PDO_OPS"] = "torch"
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    from paddle_operator_amd.ops.optim import FlatAdamW
    from paddle_operator_amd.parallel.flat import ALIGN, FlatParams

    model = GPT2(GPT2Config.named("gpt2-tiny"))
    flat = FlatParams(model, dtype=torch.float32, device="cpu", late=("wte",), split=("wte",))
    opt = FlatAdamW(flat)
    wte = dict(model.named_parameters())["wte.weight"] if "wte.weight" in dict(model.named_parameters()) else None
    head = flat.legacy_head_elems(flat.numel + sum((a.numel + ALIGN - 1) // ALIGN * ALIGN for a in flat.aux_slots))
    assert head > 0 and (wte is None or head >= wte.numel())
    new = torch.randn(flat.numel)
    legacy = torch.cat([torch.full((head,), 7.0), new])
    flat.load_params(legacy)
    assert torch.equal(flat.params, new)
    opt.load_state_dict({"master": legacy, "m": legacy * 2, "v": legacy.abs(), "step": 3})
    assert torch.equal(opt.master, new) and torch.equal(opt.m, new * 2) and opt.step_count == 3
    flat.load_params(new * 3)  # the current layout
    assert torch.equal(flat.params, new * 3)
    with pytest.raises(ValueError):
        flat.load_params(torch.zeros(flat.numel + 1))

