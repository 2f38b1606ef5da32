"""The CTR sparse path without a GPU: the references of csrc/hip/ctr.hip's rules
(ops/ctr.py), the trainer on the reference path, and the launcher in Single mode."""
import re

import pytest
import torch
import torch.nn.functional as F

from test_ctr_gpu import (PATTERNS, _port, _rank_worker, assert_same_state, dense_reference_step, exact64, grid,
                          grid_case, id_pattern, same_bits, spawn_ranks)
from test_launch import launch, records, wait_all

from paddle_operator_amd.models.wide_deep import WideDeep, WideDeepConfig
from paddle_operator_amd.ops.ctr import (ADAGRAD, GRAD, ctr_lookup, ctr_sparse_step, ref_ctr_lookup,
                                         ref_ctr_sparse_step, ref_run_sums)
from paddle_operator_amd.workloads.ctr import CTRTrainer, auc_from_scores


# ----------------------------------------------------------------------------- 1: the grid
@pytest.mark.parametrize("name", PATTERNS)
def test_grid_makes_run_sums_exact(name):
    """On the dyadic inputs of the exact GPU tests fp32 and float64 give the same bits:
    every intermediate fits 24 bits, so neither order nor FMA contraction can show."""
    c = grid_case(name)
    for ssum in (None, c["ssum"]):
        u32, G32, W32 = ref_run_sums(c["ids"], c["dX"], c["dlogit"], ssum, c["deep"])
        u64, G64, W64 = ref_run_sums(c["ids"], c["dX"].double(), c["dlogit"].double(),
                                     None if ssum is None else ssum.double(), c["deep"].double())
        assert torch.equal(u32, u64) and exact64(G32, G64) and exact64(W32, W64)
        # the kernel's form of the same sum: Σ dX, Σ dlogit·ssum and e·Σ dlogit on their own
        B, S = c["ids"].shape
        flat = c["ids"].reshape(-1)
        ok = (flat >= 0) & (flat < c["rows"])
        inv = torch.unique(flat[ok], return_inverse=True)[1]
        for dt in (torch.float32, torch.float64):
            dl = c["dlogit"].to(dt).repeat_interleave(S)[ok]
            a = torch.zeros(len(u64), c["D"], dtype=dt).index_add_(0, inv, c["dX"].to(dt).reshape(B * S, -1)[ok])
            sd = torch.zeros(len(u64), dtype=dt).index_add_(0, inv, dl)
            g = a
            if ssum is not None:
                t = torch.zeros_like(a).index_add_(0, inv, dl[:, None] * ssum.to(dt).repeat_interleave(S, 0)[ok])
                g = (a + t) - c["deep"].to(dt)[u64] * sd[:, None]
            assert exact64(g.float(), G64) and exact64(sd.float(), W64)


@pytest.mark.parametrize("shape", [(40, 26, 16), (700, 2, 16), (65, 5, 64)])
def test_grid_makes_forward_sums_exact(shape):
    B, S, D = shape
    gen = torch.Generator().manual_seed(B)
    ids = torch.randint(0, 37, (B, S), generator=gen)
    deep, wide, dense = grid(gen, (37, D)), grid(gen, (37,)), grid(gen, (B, 2))
    r32 = ref_ctr_lookup(ids, dense, deep, wide, True)
    r64 = ref_ctr_lookup(ids, dense.double(), deep.double(), wide.double(), True)
    for a, b in zip(r32, r64):
        assert exact64(a, b)


# ----------------------------------------------------------------------------- 2: sparse = dense
@pytest.mark.parametrize("model", ["wide_deep", "deepfm"])
def test_reference_sparse_step_equals_dense_autograd(model):
    cfg = WideDeepConfig(n_sparse=5, vocab_per_slot=6, emb_dim=8, n_dense=3, hidden=(16, 8), model=model)
    torch.manual_seed(1)
    m = WideDeep(cfg).double()
    with torch.no_grad():
        m.wide.weight.normal_()
        m.deep_emb.weight.mul_(30)
    gen = torch.Generator().manual_seed(2)
    B = 9
    ids = torch.randint(0, 4, (B, cfg.n_sparse), generator=gen) + torch.arange(cfg.n_sparse) * cfg.vocab_per_slot
    dense = torch.rand(B, cfg.n_dense, generator=gen).double()
    label = (torch.rand(B, generator=gen) > 0.5).double()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    logit_d, loss_d, deep_d, wide_d = dense_reference_step(sd, cfg, ids, dense, label, torch.float64, 0.05)

    deep, wide = sd["deep_emb.weight"].clone(), sd["wide.weight"].clone()
    acc_d, acc_w = torch.full_like(deep, 0.1), torch.full_like(wide, 0.1)
    fm = model == "deepfm"
    X, ws, fmt, ssum = ref_ctr_lookup(ids, dense, deep, wide, fm)
    X.requires_grad_(True)
    ws.requires_grad_(True)
    logit = m.tower.logit_from_lookup(X, ws, fmt)
    loss = F.binary_cross_entropy_with_logits(logit, label)
    loss.backward()
    assert (logit.detach() - logit_d).abs().max() < 1e-12 and abs(float(loss.detach()) - float(loss_d)) < 1e-12
    ref_ctr_sparse_step(ids, X.grad, ws.grad, ssum, (deep, wide), (acc_d, acc_w), 0.05, ADAGRAD)
    assert (deep - deep_d).abs().max() < 1e-12 and (wide - wide_d).abs().max() < 1e-12
    rest = torch.ones(cfg.rows, dtype=torch.bool)
    rest[torch.unique(ids)] = False
    assert rest.any()
    assert torch.equal(deep[rest], sd["deep_emb.weight"][rest]) and torch.equal(wide[rest], sd["wide.weight"][rest])
    assert (acc_d[rest] == 0.1).all() and (acc_w[rest] == 0.1).all()
    # GRAD mode gives the dense gradient's rows
    g_deep, g_wide = torch.zeros_like(deep), torch.zeros_like(wide)
    ref_ctr_sparse_step(ids, X.grad, ws.grad, ssum, (sd["deep_emb.weight"], sd["wide.weight"]), (g_deep, g_wide),
                        None, GRAD)
    m2 = WideDeep(cfg).double()
    m2.load_state_dict(sd)
    F.binary_cross_entropy_with_logits(m2(ids, dense), label).backward()
    assert (g_deep - m2.deep_emb.weight.grad).abs().max() < 1e-12
    assert (g_wide - m2.wide.weight.grad).abs().max() < 1e-12


# ----------------------------------------------------------------------------- 3: launcher
def test_launcher_single_mode_trains_deepfm(tmp_path):
    """Without pserver endpoints the launcher builds the trainer and trains (before, it
    reported ready and exited without a step)."""
    log = tmp_path / "run.log"
    p = launch({}, ["--workload", "deepfm", "--tiny", "--steps", "30", "--eval-every", "10", "--log-every", "1"], log)
    assert wait_all([p]) == [0], open(log).read()[-3000:]
    evals = records(log, "PDO_EVAL")
    assert [e["step"] for e in evals] == [10, 20, 30]
    assert all(0.0 <= e["auc"] <= 1.0 and e["val_loss"] > 0 for e in evals)
    done = records(log, "PDO_DONE")
    assert done and done[0]["steps"] == 30 and done[0]["throughput"] > 0
    text = open(log).read()
    assert "samples/s" in text
    losses = [float(x) for x in re.findall(r"step \d+/30 loss ([0-9.]+)", text)]
    assert len(losses) == 30
    assert sum(losses[-10:]) / 10 < sum(losses[:10]) / 10


# ----------------------------------------------------------------------------- 4: resume
@pytest.mark.parametrize("model", ["wide_deep", "deepfm"])
def test_resume_replays_bit_for_bit(tmp_path, model):
    from paddle_operator_amd.utils import checkpoint as ckpt
    cfg = WideDeepConfig(vocab_per_slot=50, model=model)

    def make():
        return CTRTrainer(cfg, 32, "cpu", data_seed=5)
    a = make()
    la = [float(a.step()) for _ in range(6)]
    b = make()
    lb = [float(b.step()) for _ in range(3)]
    ckpt.save(b.state_dict(), str(tmp_path), 3)
    st, step = ckpt.load_latest(str(tmp_path))
    c = make()
    c.load_state_dict(st)
    assert step == 3 and c.step_count == 3
    lb += [float(c.step()) for _ in range(3)]
    assert la == lb
    assert_same_state(a.state_dict(), c.state_dict())  # tables, accumulators, tower, Adam moments and step
    m = WideDeep(cfg)
    m.load_state_dict(st["model"])


# ----------------------------------------------------------------------------- 5: two gloo ranks
def _recording_worker(rank, world, port, outdir):
    """_rank_worker on the CPU that also records the first sparse step's arguments."""
    import os

    from paddle_operator_amd.workloads import ctr as wl
    real = wl.ctr_ops.ctr_sparse_step
    seen = []

    def spy(ids, dX, dlogit, ssum, tables, accs, lr, mode):
        if not seen:
            before = [t.clone() for t in (*tables, *accs)]
        real(ids, dX, dlogit, ssum, tables, accs, lr, mode)
        if not seen:
            seen.append(1)
            torch.save({"ids": ids, "dX": dX.clone(), "dlogit": dlogit.clone(), "ssum": ssum.clone(), "lr": lr.clone(),
                        "before": before, "after": [t.clone() for t in (*tables, *accs)]},
                       os.path.join(outdir, f"first{rank}.pt"))
    wl.ctr_ops.ctr_sparse_step = spy
    _rank_worker(rank, world, port, outdir, "cpu", "deepfm")


def test_two_gloo_ranks_keep_replicas_identical(tmp_path):
    spawn_ranks(_recording_worker, (2, _port(), str(tmp_path)), 2)
    r = [torch.load(tmp_path / f"r{k}.pt", weights_only=True) for k in range(2)]
    assert_same_state({k: v for k, v in r[0]["state"].items() if k != "adam"},
                      {k: v for k, v in r[1]["state"].items() if k != "adam"})
    f = [torch.load(tmp_path / f"first{k}.pt", weights_only=True) for k in range(2)]
    for k in ("ids", "dX", "dlogit", "ssum"):
        assert same_bits(f[0][k].float(), f[1][k].float()), k
    # rank order: the first B rows are rank 0's batch, the next B rank 1's
    cfg = WideDeepConfig(vocab_per_slot=1000, model="deepfm")
    tr = CTRTrainer(cfg, 64, "cpu")
    for rank in range(2):
        assert torch.equal(f[0]["ids"][64 * rank:64 * (rank + 1)], tr.draw(0, 0, rank)[0])
    deep, wide, acc_d, acc_w = (t.clone() for t in f[0]["before"])
    ref_ctr_sparse_step(f[0]["ids"], f[0]["dX"], f[0]["dlogit"], f[0]["ssum"], (deep, wide), (acc_d, acc_w),
                        f[0]["lr"], ADAGRAD)
    for got, want in zip(f[0]["after"], (deep, wide, acc_d, acc_w)):
        assert same_bits(got, want)
    for a, b in zip(f[0]["after"], f[1]["after"]):
        assert same_bits(a, b)


# ----------------------------------------------------------------------------- 6: contract
@pytest.mark.parametrize("D", [6, 68])
def test_contract_refuses_row_width(D):
    ids = torch.zeros(2, 3, dtype=torch.int64)
    deep, wide = torch.zeros(4, D), torch.zeros(4)
    with pytest.raises(ValueError):
        ctr_lookup(ids, torch.zeros(2, 0), deep, wide, False)
    with pytest.raises(ValueError):
        ctr_sparse_step(ids, torch.zeros(2, 3 * D), torch.zeros(2), None, (deep, wide),
                        (torch.zeros_like(deep), torch.zeros_like(wide)), 0.1, ADAGRAD)


def test_out_of_range_ids_read_zeros_and_update_nothing():
    ids, rows, D = id_pattern("oor")
    B, S = ids.shape
    gen = torch.Generator().manual_seed(0)
    deep, wide = torch.randn(rows, D, generator=gen), torch.randn(rows, generator=gen)
    X, ws, fm, ssum = ctr_lookup(ids, torch.zeros(B, 0), deep, wide, True)
    bad = (ids < 0) | (ids >= rows)
    assert bad.any() and not X.reshape(B, S, D)[bad].any()
    only_bad = torch.where(bad, ids, torch.full_like(ids, -7))  # every lookup outside the table
    d2, w2, a_d, a_w = deep.clone(), wide.clone(), torch.full_like(deep, 0.1), torch.full_like(wide, 0.1)
    ctr_sparse_step(only_bad, torch.ones(B, S * D), torch.ones(B), ssum, (d2, w2), (a_d, a_w), 0.1, ADAGRAD)
    assert torch.equal(d2, deep) and torch.equal(w2, wide) and (a_d == 0.1).all() and (a_w == 0.1).all()
    X0, ws0, fm0, _ = ctr_lookup(only_bad, torch.zeros(B, 0), deep, wide, True)
    assert not X0.any() and not ws0.any() and not fm0.any()


def test_auc_by_one_sort_matches_pair_counting():
    gen = torch.Generator().manual_seed(4)
    s = torch.randint(0, 12, (200,), generator=gen).float()  # many ties
    y = (torch.rand(200, generator=gen) > 0.6).float()
    u, pairs = auc_from_scores(s, y).tolist()
    pos, neg = s[y == 1], s[y == 0]
    want = ((pos[:, None] > neg[None, :]).double() + 0.5 * (pos[:, None] == neg[None, :]).double()).sum()
    assert pairs == len(pos) * len(neg) and abs(u - float(want)) < 1e-9
