"""Training step engine shared by ``bench.py``, ``pdo-launch`` workloads and tests.

One step = zero grads (memset of the flat arena) → forward → backward with
bucketed RCCL all-reduce overlapped → fused AdamW.  Synthetic batches are
generated on device every step (``torch.randint`` on the GPU; no H2D copy),
matching BASELINE's "synthetic data / random-init weights" rule.  With ``data=`` the
batches are windows of a uint16 token file (``data.py``); ``grad_accum=K`` runs K
micro-batches per optimizer step through an fp32 accumulator; ``evaluate()`` measures
the held-out loss.  With none of these given the step is the one described above.
"""
from __future__ import annotations

import contextlib
import os
import time
from dataclasses import dataclass

import torch
import torch.distributed as dist

from .models.gpt2 import GPT2, GPT2Config
from .ops import deferred_reductions, deferred_weight_grads
from .ops.optim import FlatAdamW, cosine_lr
from .parallel.ddp import BucketedDDP
from .parallel.flat import FlatParams
from .utils import trace
from .utils.topology import bucket_bytes_for


@dataclass
class DistInfo:
    rank: int = 0
    world: int = 1
    local_rank: int = 0

    @property
    def is_main(self):
        return self.rank == 0


def init_distributed(backend: str | None = None, timeout_s: int = 600) -> DistInfo:
    """Initialise torch.distributed from the torchrun / pdo-launch env contract.

    On ROCm the ``nccl`` backend IS RCCL.  ``hipSetDevice(local_rank)`` happens
    before any other HIP call so the communicator binds the right GPU.
    """
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    info = DistInfo(rank, world, local)
    # PDO_DIST_BACKEND=gloo rehearses the multi-rank GPU path with every rank on
    # one device (RCCL refuses two ranks per GPU); production is nccl = RCCL
    backend = backend or os.environ.get("PDO_DIST_BACKEND") or None
    if torch.cuda.is_available():
        ndev = torch.cuda.device_count()
        if backend == "gloo" and local >= ndev:
            local = local % ndev
            info.local_rank = local
        torch.cuda.set_device(local)
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    # RCCL comes up eagerly even at world 1 (device_id → communicator built
    # now, so "ready" includes comm init and the DDP path is the one that runs
    # at scale); a CPU world of 1 needs no process group
    if (world > 1 or backend == "nccl") and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        kw = {}
        if backend == "nccl":
            kw["device_id"] = torch.device("cuda", local)
        if world == 1 and "MASTER_PORT" not in os.environ:
            kw["store"] = dist.HashStore()  # single rank: no rendezvous port
        import datetime
        dist.init_process_group(backend, rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=timeout_s), **kw)
    return info


def derive_dropout_seed(dropout_seed: int, rank: int) -> int:
    """The 64-bit dropout key of one rank: the splitmix64 finaliser of
    ``dropout_seed + (rank + 1)·0x9E3779B97F4A7C15`` (mod 2^64).  Deterministic in
    (dropout_seed, rank), and ranks of one job draw different masks."""
    m = (1 << 64) - 1
    z = (int(dropout_seed) + (int(rank) + 1) * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


# test hook (not a user knob): False adds every micro-batch of an accumulated step
# straight into the bf16 arena, without the fp32 accumulator
_ACCUM_FP32 = [True]


class GPT2Trainer:
    """``grad_accum=K`` > 1: one ``step()`` runs K micro-batches of ``micro_batch`` rows
    (each loss × 1/K, the first K − 1 under ``ddp.no_sync()``, the last with the
    overlapped bucketed all-reduce) and one optimizer step.  Micro-batches 1 … K − 1 are
    summed in fp32 (``grad_accum_fold``, csrc/hip/bucket.hip) and handed back to the
    bf16 arena just before micro-batch K, whose kernels add into the arena directly.

    ``data`` / ``val_data``: uint16 token files (``data.py``); without ``data`` the
    batches are synthetic.  ``lr_schedule="cosine"``: the rate of an optimizer step is
    ``cosine_lr(opt.step_count, lr, lr_warmup, lr_decay_steps, lr_min_ratio)``."""

    def __init__(self, cfg: GPT2Config, micro_batch: int, seq_len: int, device,
                 dtype=torch.bfloat16, lr=3e-4, bucket_mb: int | None = None, seed: int = 0,
                 dropout_seed: int = 0, grad_accum: int = 1, data: str | None = None, val_data: str | None = None,
                 data_seed: int = 0, data_device_gb: float = 8.0, lr_schedule: str = "constant",
                 lr_warmup: int = 0, lr_decay_steps: int = 10000, lr_min_ratio: float = 0.1):
        if grad_accum < 1:
            raise ValueError(f"grad_accum must be at least 1, not {grad_accum}")
        if lr_schedule not in ("constant", "cosine"):
            raise ValueError(f"lr_schedule must be constant or cosine, not {lr_schedule!r}")
        self.K = int(grad_accum)
        self.lr_schedule = lr_schedule
        self.lr_warmup, self.lr_decay_steps, self.lr_min_ratio = int(lr_warmup), int(lr_decay_steps), lr_min_ratio
        self.cfg = cfg
        self.B = micro_batch
        self.S = seq_len
        self.device = torch.device(device)
        if self.device.type == "cuda":
            from .utils.tuning import enable_tuned_gemms
            enable_tuned_gemms()
        torch.manual_seed(seed)
        if self.device.type == "cuda":
            # built and initialised on the device (models/gpt2.py reset_parameters)
            with torch.device(self.device):
                model = GPT2(cfg)
        else:
            model = GPT2(cfg)
        model.to(device=self.device, dtype=dtype)
        self.model = model
        if bucket_mb is None:
            world = dist.get_world_size() if dist.is_initialized() else 1
            nbytes = sum(p.numel() for p in model.parameters()) * torch.empty((), dtype=dtype).element_size()
            bucket_bytes = bucket_bytes_for(world, nbytes)
        else:
            bucket_bytes = bucket_mb << 20
        # the tied wte gradient in two slots: the LM-head half is bucket 0 (its
        # all-reduce overlaps the whole backward), the embedding half the last
        # bucket (PDO_SPLIT_WTE=0: one slot, all of it in the last bucket)
        split = ("wte",) if os.environ.get("PDO_SPLIT_WTE", "1") != "0" else ()
        self.flat = FlatParams(model, dtype=dtype, device=self.device, bucket_bytes=bucket_bytes, late=("wte",),
                               split=split)
        # every dX GEMM's Wᵀ operand built in one launch per step (wt_scope)
        self.flat.enable_wt()
        self.ddp = BucketedDDP(self.flat)
        self.opt = FlatAdamW(self.flat, lr=lr)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed + (dist.get_rank() if dist.is_initialized() else 0))
        # dropout (cfg.*_pdrop): masks are a function of (seed, step, site, element);
        # drop_step advances once per step() and is part of the checkpoint
        model.drop_seed = derive_dropout_seed(dropout_seed, dist.get_rank() if dist.is_initialized() else 0)
        self.drop_step = 0
        # token files: the micro-batch counter of the training stream (data.py) advances
        # once per micro-batch and is the only loader state in the checkpoint
        self.data_step = 0
        self.data = self.val = None
        rank = dist.get_rank() if dist.is_initialized() else 0
        if data:
            from .data import TRAIN_STREAM, TokenStream
            self.data = TokenStream(data, self.B, self.S, cfg.vocab_size, self.device, data_seed, TRAIN_STREAM, rank,
                                    data_device_gb)
        if val_data:
            from .data import EVAL_STREAM, TokenStream
            self.val = TokenStream(val_data, self.B, self.S, cfg.vocab_size, self.device, data_seed, EVAL_STREAM,
                                   rank, data_device_gb)
        # fp32 sum of micro-batches 1 … K − 1: 4 B per gradient element, only for K > 2
        # (at K = 2 the arena already holds micro-batch 1 when micro-batch 2 adds into it)
        self.acc = torch.zeros(self.flat.grads.numel(), dtype=torch.float32, device=self.device) if self.K > 2 else None

    def sync_initial_weights(self):
        self.ddp.broadcast_params(0)
        self.opt.master.copy_(self.flat.params.float())

    def batch(self):
        if self.data is not None:
            return self.data.batch(self.data_step)
        V = self.cfg.vocab_size
        idx = torch.randint(0, V, (self.B, self.S + 1), device=self.device, generator=self.gen)
        return idx[:, :-1], idx[:, 1:]

    def next_lr(self) -> float:
        """The rate of the next optimizer step (``opt.step_count`` steps taken so far)."""
        if self.lr_schedule == "cosine":
            return cosine_lr(self.opt.step_count, self.opt.lr, self.lr_warmup, self.lr_decay_steps, self.lr_min_ratio)
        return self.opt.lr

    def step(self, idx=None, tgt=None):
        if self.K > 1:
            return self._step_accum(idx, tgt)
        if idx is None:
            idx, tgt = self.batch()
        self.model.drop_step = self.drop_step & 0xFFFFFFFF
        self.drop_step += 1
        self.data_step += 1
        self.flat.zero_grad()
        self.ddp.prepare()
        with self.flat.wt_scope():
            with trace.range("forward"):
                loss = self.model(idx, tgt)
            # bias / norm-weight column sums batched (flushed before each bucket
            # all-reduce and at the end of the backward)
            # (and the arena dW GEMMs grouped into whole rounds, ops.core deferred_weight_grads)
            with trace.range("backward"), deferred_reductions(self.device), deferred_weight_grads(self.device):
                loss.backward()
        with trace.range("allreduce_drain"):
            self.ddp.finish(self.opt if self.opt.max_grad_norm else None)
        with trace.range("optimizer"):
            self.opt.step(grad_scale=self.ddp.grad_scale, lr=self.next_lr())
        return loss

    def _step_accum(self, idx, tgt):
        """One optimizer step over K micro-batches (class docstring).  ``idx`` / ``tgt``
        of K·B rows are run as K chunks of B."""
        K, B = self.K, self.B
        if idx is not None and idx.shape[0] != K * B:
            raise ValueError(f"step(idx, tgt) with grad_accum={K} takes {K * B} rows, got {idx.shape[0]}")
        losses = []
        self.flat.zero_grad()
        # the weights do not change between micro-batches: one set of Wᵀ operands
        with self.flat.wt_scope():
            for i in range(1, K + 1):
                x, y = (idx[(i - 1) * B:i * B], tgt[(i - 1) * B:i * B]) if idx is not None else self.batch()
                self.model.drop_step = self.drop_step & 0xFFFFFFFF
                self.drop_step += 1
                self.data_step += 1
                self.ddp.prepare()
                with contextlib.nullcontext() if i == K else self.ddp.no_sync():
                    with trace.range("forward"):
                        loss = self.model(x, y)
                    with trace.range("backward"), deferred_reductions(self.device), \
                            deferred_weight_grads(self.device):
                        (loss * (1.0 / K)).backward()
                    # after finish the split LM-head slot is folded into its gradient and zero
                    with trace.range("allreduce_drain"):
                        self.ddp.finish(self.opt if self.opt.max_grad_norm and i == K else None)
                losses.append(loss.detach())
                if self.acc is not None and _ACCUM_FP32[0] and i < K:
                    self._fold(init=(i == 1), emit=(i == K - 1))
        with trace.range("optimizer"):
            self.opt.step(grad_scale=self.ddp.grad_scale, lr=self.next_lr())
        return torch.stack(losses).mean()

    def _fold(self, init: bool, emit: bool):
        """acc = (init ? 0 : acc) + f32(arena); arena = emit ? bf16(acc) : 0."""
        g = self.flat.grads
        if g.is_cuda and g.dtype == torch.bfloat16:
            from . import _native
            _native.require_hip().grad_accum_fold(g, self.acc, init, emit)
            return
        if init:
            self.acc.zero_()
        self.acc.add_(g.float())
        if emit:
            g.copy_(self.acc)
        else:
            g.zero_()

    @torch.no_grad()
    def evaluate(self, n_batches: int) -> float:
        """Mean held-out loss over micro-batches 0 … n_batches − 1 of the evaluation
        stream of ``val_data`` — the same windows at every call — summed over ranks.
        Runs in eval mode (no dropout) on the loss-only LM head; touches neither the
        counters, the gradient arena nor the optimizer."""
        if self.val is None:
            raise RuntimeError("evaluate() needs val_data")
        was_training = self.model.training
        self.model.eval()
        try:
            tot = torch.zeros(2, dtype=torch.float64, device=self.device)  # Σ loss·count, Σ count
            for m in range(n_batches):
                idx, tgt = self.val.batch(m)
                loss = self.model(idx, tgt)
                cnt = (tgt >= 0).sum()
                tot[0] += loss.double() * cnt
                tot[1] += cnt
            if dist.is_initialized() and dist.get_world_size() > 1:
                if dist.get_backend() == "nccl":
                    dist.all_reduce(tot)
                else:
                    t = tot.cpu()
                    dist.all_reduce(t)
                    tot = t
        finally:
            self.model.train(was_training)
        self.check_data()
        return float(tot[0] / tot[1].clamp(min=1))

    def check_data(self):
        """Raise if a token file fed an id ≥ vocab_size.  Reads a device counter: call
        where the step is synchronised anyway (log line, evaluation, checkpoint, end)."""
        for d in (self.data, self.val):
            if d is not None:
                d.check()

    def close(self):
        for d in (self.data, self.val):
            if d is not None:
                d.close()

    def tokens_per_step(self):
        return self.B * self.S * self.K

    def state_dict(self):
        self.check_data()
        return {"params": self.flat.params, "opt": self.opt.state_dict(), "drop_step": self.drop_step,
                "data_step": self.data_step}

    def load_state_dict(self, st, step: int = 0):
        """``step``: the resumed step number, where the dropout stream starts for a
        checkpoint written before ``drop_step`` existed and, times ``grad_accum``, the
        data stream for one written before ``data_step``."""
        self.flat.load_params(st["params"])
        self.opt.load_state_dict({k: v.to(self.device) if torch.is_tensor(v) else v for k, v in st["opt"].items()})
        self.drop_step = int(st.get("drop_step", step))
        self.data_step = int(st.get("data_step", step * self.K))


def now():
    return time.perf_counter()
