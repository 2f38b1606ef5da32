"""Wide&Deep / DeepFM training in Collective and Single mode (``CTRTrainer``).

The sparse side — the lookup of the batch's ``B × S`` rows with the wide sum and
DeepFM's second-order term, and the backward that sums the per-lookup gradients
and applies row-wise Adagrad to the rows the batch touched — runs on
``ops.ctr_lookup`` / ``ops.ctr_sparse_step`` (``csrc/hip/ctr.hip`` on the GPU, the
torch reference on CPU tensors and under ``PDO_OPS=torch``).  The dense tower stays
on torch in fp32 with Adam, as in ``parallel.ps.ShardServer``.

Without ``data`` the batches are synthetic and drawn on the device from a generator
reseeded for every step from ``(data_seed, step counter, rank)`` alone, with the label
rule of ``models.wide_deep.synthetic_batch``.  With ``data`` / ``val_data`` they come from
click directories (``data.ClickStream``, ``data.CLICK_DOC``): one launch of
``csrc/hip/click.hip`` draws the batch's records, hashes the raw categorical values into
table rows and normalises the dense features.  Either way a batch is a function of
``(data_seed, step counter, rank)``, and the step counter is in the checkpoint, so a
resumed job replays the batches the uninterrupted one would have seen.

More than one rank: the tables are replicas.  A step all-gathers ``ids``, ``dX``,
``dlogit`` (already scaled by ``1 / (world·B)``) and ``ssum`` and every rank runs the
sparse step over the concatenation in rank order — the replicas stay bit-identical
and no dense table travels; the tower's gradients are all-reduced.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn.functional as F

from ..models.wide_deep import WideDeepConfig, make_tower
from ..ops import ctr as ctr_ops

TRAIN_STREAM, EVAL_STREAM = 0, 1
_M63 = (1 << 63) - 1


def batch_seed(data_seed: int, stream: int, step: int, rank: int) -> int:
    """The generator seed of one batch: a fixed mix of its four coordinates."""
    x = (int(data_seed) * 0x9E3779B97F4A7C15 + int(step) * 0xBF58476D1CE4E5B9 + int(rank) * 0x94D049BB133111EB
         + int(stream) * 0xD6E8FEB86659FD93 + 0x2545F4914F6CDD1D)
    x ^= x >> 31
    return x & _M63


def auc_from_scores(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """``[U, n_pos·n_neg]`` (float64) of the Mann-Whitney statistic by one sort, ties at
    their mid-rank; AUC = U / (n_pos·n_neg).  Both numbers add up over ranks' shares."""
    s, order = torch.sort(scores.double())
    y = labels[order].double()
    _, inv, cnt = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
    end = torch.cumsum(cnt, 0).double()  # 1-based rank of the last of each tie group
    mid = (end - (cnt.double() - 1.0) / 2.0)[inv]
    n_pos = y.sum()
    n_neg = y.numel() - n_pos
    u = (mid * y).sum() - n_pos * (n_pos + 1.0) / 2.0
    return torch.stack([u, n_pos * n_neg])


class CTRTrainer:
    def __init__(self, cfg: WideDeepConfig, batch: int, device, lr: float = 1e-3, sparse_lr: float = 0.05,
                 data_seed: int = 0, eval_seed: int | None = None, seed: int = 0, data: str | None = None,
                 val_data: str | None = None, data_device_gb: float = 8.0):
        self.cfg = cfg
        self.device = torch.device(device)
        self.B = int(batch)
        self.fm = cfg.model == "deepfm"
        self.rank, self.world = (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)
        g = torch.Generator().manual_seed(seed)
        dev = self.device
        # the tables and their Adagrad accumulators (ShardServer's initial values)
        self.deep = (torch.randn(cfg.rows, cfg.emb_dim, generator=g) * 0.01).to(dev)
        self.wide = torch.zeros(cfg.rows, 1, device=dev)
        self.deep_acc = torch.full((cfg.rows, cfg.emb_dim), 0.1, device=dev)
        self.wide_acc = torch.full((cfg.rows, 1), 0.1, device=dev)
        torch.manual_seed(seed)
        self.tower = make_tower(cfg).to(dev)
        self.opt = torch.optim.Adam(self.tower.parameters(), lr=lr)
        self.sparse_lr = float(sparse_lr)
        self.lr_dev = torch.full((1,), self.sparse_lr, dtype=torch.float32, device=dev)
        self.data_seed = int(data_seed)
        self.eval_seed = int(data_seed) + 1 if eval_seed is None else int(eval_seed)
        self.step_count = 0
        self.gen = torch.Generator(device=dev)
        self._slot_base = (torch.arange(cfg.n_sparse, device=dev) * cfg.vocab_per_slot)
        self.K = ctr_ops.min_ldx(cfg.n_sparse, cfg.emb_dim, cfg.n_dense)
        # rows of X and dX on 16 B for the kernels' vector accesses; the torch path needs no padding
        self.ldx = ctr_ops.padded_ldx(cfg.n_sparse, cfg.emb_dim, cfg.n_dense) if ctr_ops.use_hip(self.deep) else self.K
        # click directories (data.ClickStream); the validation set is normalised with the training set's stats
        self.train = self.val = None
        if data or val_data:
            from ..data import ClickStream
            common = dict(seed=self.data_seed, rank=self.rank, world=self.world, device_gb=data_device_gb)
            shape = (self.B, cfg.n_sparse, cfg.n_dense, cfg.vocab_per_slot, dev)
            if data:
                self.train = ClickStream(data, *shape, stream=TRAIN_STREAM, **common)
            if val_data:
                self.val = ClickStream(val_data, *shape, stream=EVAL_STREAM,
                                       stats=self.train.stats if self.train is not None else None, **common)

    # ------------------------------------------------------------------ data
    def draw(self, stream: int, step: int, rank: int | None = None):
        """Batch ``step`` of a stream: ``(ids [B, S], dense [B, n_dense], label [B])`` on the
        device, a function of ``(seed, stream, step, rank)`` only.  With ``data`` / ``val_data``
        the stream's batches come from the click directory (this rank's rows; on the validation
        stream a row past the end of the set has ids −1 and label −1)."""
        files = self.train if stream == TRAIN_STREAM else self.val
        if files is not None:
            if rank is not None and rank != self.rank:
                raise ValueError(f"draw: a click stream serves its own rank {self.rank}, not {rank}")
            return files.batch(step)
        cfg = self.cfg
        seed = self.data_seed if stream == TRAIN_STREAM else self.eval_seed
        self.gen.manual_seed(batch_seed(seed, stream, step, self.rank if rank is None else rank))
        dev = self.device
        slot_ids = torch.randint(0, cfg.vocab_per_slot, (self.B, cfg.n_sparse), generator=self.gen, device=dev)
        ids = slot_ids + self._slot_base
        dense = torch.rand(self.B, cfg.n_dense, generator=self.gen, device=dev)
        score = (slot_ids % 7 == 0).float().mean(1) * 4 + dense[:, 0] - 1.0
        label = (score + 0.1 * torch.randn(self.B, generator=self.gen, device=dev) > 0).float()
        return ids, dense, label

    # ------------------------------------------------------------------ step
    def forward(self, ids, dense):
        """``(logit, X, wide_sum, fm_term, ssum)``; ``X`` and ``wide_sum`` are leaves whose
        ``.grad`` after a backward are ``dX`` and ``dlogit``."""
        X, ws, fmt, ssum = ctr_ops.ctr_lookup(ids, dense, self.deep, self.wide, self.fm, self.ldx)
        X.requires_grad_(True)
        ws.requires_grad_(True)
        logit = self.tower.logit_from_lookup(X[:, :self.K], ws, fmt)
        return logit, X, ws, fmt, ssum

    def _gather(self, t: torch.Tensor) -> torch.Tensor:
        """The ranks' tensors concatenated along dim 0 in rank order."""
        if self.world == 1:
            return t
        via_host = t.is_cuda and dist.get_backend() != "nccl"
        src = t.contiguous().cpu() if via_host else t.contiguous()
        parts = [torch.empty_like(src) for _ in range(self.world)]
        dist.all_gather(parts, src)
        return torch.cat(parts, 0).to(t.device)

    def _reduce_tower_grads(self):
        if self.world == 1:
            return
        grads = [p.grad for p in self.tower.parameters()]
        flat = torch.cat([g.reshape(-1) for g in grads])
        via_host = flat.is_cuda and dist.get_backend() != "nccl"
        buf = flat.cpu() if via_host else flat
        dist.all_reduce(buf)
        flat = buf.to(grads[0].device)
        o = 0
        for g in grads:
            g.copy_(flat[o:o + g.numel()].view_as(g))
            o += g.numel()

    def step(self):
        """One training step; returns this rank's mean loss (detached)."""
        ids, dense, label = self.draw(TRAIN_STREAM, self.step_count)
        self.opt.zero_grad(set_to_none=True)
        logit, X, ws, _, ssum = self.forward(ids, dense)
        loss_sum = F.binary_cross_entropy_with_logits(logit, label, reduction="sum")
        (loss_sum / (self.world * self.B)).backward()  # the mean over the global batch
        self._reduce_tower_grads()
        self.opt.step()
        with torch.no_grad():
            ctr_ops.ctr_sparse_step(self._gather(ids), self._gather(X.grad), self._gather(ws.grad),
                                    self._gather(ssum) if self.fm else None, (self.deep, self.wide),
                                    (self.deep_acc, self.wide_acc), self.lr_dev, ctr_ops.ADAGRAD)
        self.step_count += 1
        return (loss_sum / self.B).detach()

    def sync_initial_weights(self):
        if self.world == 1:
            return
        tensors = [self.deep, self.wide, self.deep_acc, self.wide_acc] + [p.data for p in self.tower.parameters()]
        for t in tensors:
            if t.is_cuda and dist.get_backend() != "nccl":
                h = t.cpu()
                dist.broadcast(h, 0)
                t.copy_(h)
            else:
                dist.broadcast(t, 0)

    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def evaluate(self, n_batches: int = 8) -> dict:
        """Held-out log-loss and AUC over batches 0 … n_batches − 1 of the validation stream
        (its own seed), summed over ranks by one all-reduce.  AUC is the rank statistic of
        one device sort per rank; over several ranks it is the pair-weighted mean of the
        ranks' AUCs (positives and negatives are paired within a rank's share).

        With ``val_data``: batches 0 … n_batches − 1 of the click directory's evaluation stream
        (0: the whole set once, ``batches_per_epoch()``).  The ranks' logits and labels are
        all-gathered, the pad rows (label −1) dropped, and loss and AUC computed over what is
        left: the exact rank statistic of the whole set.  The result gains ``"records"``."""
        if self.val is not None:
            return self._evaluate_files(int(n_batches))
        nb = max(1, int(n_batches))
        logits, labels = [], []
        for m in range(nb):
            ids, dense, label = self.draw(EVAL_STREAM, m)
            X, ws, fmt, _ = ctr_ops.ctr_lookup(ids, dense, self.deep, self.wide, self.fm, self.ldx)
            logits.append(self.tower.logit_from_lookup(X[:, :self.K], ws, fmt))
            labels.append(label)
        z, y = torch.cat(logits), torch.cat(labels)
        tot = torch.cat([F.binary_cross_entropy_with_logits(z, y, reduction="sum").double().reshape(1),
                         torch.tensor([float(y.numel())], dtype=torch.float64, device=z.device),
                         auc_from_scores(z, y)])
        if self.world > 1:
            if tot.is_cuda and dist.get_backend() != "nccl":
                t = tot.cpu()
                dist.all_reduce(t)
                tot = t
            else:
                dist.all_reduce(tot)
        loss, cnt, u, pairs = tot.tolist()
        return {"val_loss": loss / max(cnt, 1.0), "auc": u / pairs if pairs > 0 else 0.5}

    def _evaluate_files(self, n_batches: int) -> dict:
        nb = n_batches if n_batches > 0 else self.val.batches_per_epoch()
        logits, labels = [], []
        for m in range(nb):
            ids, dense, label = self.draw(EVAL_STREAM, m)
            X, ws, fmt, _ = ctr_ops.ctr_lookup(ids, dense, self.deep, self.wide, self.fm, self.ldx)
            logits.append(self.tower.logit_from_lookup(X[:, :self.K], ws, fmt))
            labels.append(label)
        z, y = self._gather(torch.cat(logits)), self._gather(torch.cat(labels))
        keep = y >= 0
        z, y = z[keep], y[keep]
        loss = float(F.binary_cross_entropy_with_logits(z, y, reduction="sum").double())
        u, pairs = auc_from_scores(z, y).tolist()
        cnt = int(y.numel())
        return {"val_loss": loss / max(cnt, 1), "auc": u / pairs if pairs > 0 else 0.5, "records": cnt}

    def close(self):
        for s in (self.train, self.val):
            if s is not None:
                s.close()

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self):
        """``model`` has the keys of ``models.wide_deep.WideDeep`` and loads into it."""
        model = {"deep_emb.weight": self.deep.detach().cpu(), "wide.weight": self.wide.detach().cpu()}
        model.update({"tower." + k: v.detach().cpu() for k, v in self.tower.state_dict().items()})
        adam = self.opt.state_dict()
        adam_state = {int(k): {n: (v.detach().cpu() if torch.is_tensor(v) else v) for n, v in s.items()}
                      for k, s in adam["state"].items()}
        return {"model": model, "deep_acc": self.deep_acc, "wide_acc": self.wide_acc,
                "adam": {"state": adam_state, "param_groups": adam["param_groups"]},
                "data_step": self.step_count}

    def load_state_dict(self, sd):
        model = sd["model"]
        self.deep.copy_(model["deep_emb.weight"])
        self.wide.copy_(model["wide.weight"])
        self.deep_acc.copy_(sd["deep_acc"])
        self.wide_acc.copy_(sd["wide_acc"])
        self.tower.load_state_dict({k[len("tower."):]: v for k, v in model.items() if k.startswith("tower.")})
        if sd.get("adam", {}).get("state"):
            self.opt.load_state_dict(sd["adam"])
        self.step_count = int(sd.get("data_step", sd.get("step", 0)))
