"""Click directories on the MI355X: the click_batch kernel against its host references — the draw,
the ids, the bits of the dense features and the labels, all exactly — the device-resident and
host-staged routes of ClickStream against each other, the binding's refusals, and the CTR trainer on
click directories: evaluate against a recount, the launcher's resume, and that both models learn a
rule planted in the records.

No tolerance appears in this file: ids and records are integers, and the dense rule is one int →
fp32 conversion, one subtraction and one IEEE division, which numpy's float32 rounds the same way.
"""
import numpy as np
import pytest
import torch

from test_click_data_cpu import DENSE_EDGES, MISSING, STATS_EDGES, learnable_clicks, write_clicks

pytestmark = pytest.mark.gpu

SEED = 0xFEDC_BA98_7654_3210  # high bits set
DRAWS = ((0, 0, 0), (0, 1, 1), (0, 2**32 + 3, 3), (1, 0, 0))  # (stream, m, rank)


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _set(n, S, nd, seed):
    rng = np.random.default_rng(seed)
    cat = rng.integers(0, 2**32, (n, S), dtype=np.uint64).astype(np.uint32)
    dense = rng.integers(-1000, 100000, (n, nd)).astype(np.int32)
    dense[rng.random((n, nd)) < 0.2] = MISSING
    label = rng.integers(0, 2, n).astype(np.uint8)
    stats = np.stack([rng.integers(-1000, 10, nd), rng.integers(1, 100000, nd)]).astype(np.float32)
    return cat, dense, label, stats


def _launch(arrays, n, B, V, draw, Bg, cuda, staged=False):
    cat, dense, label, stats = arrays
    S, nd = cat.shape[1], dense.shape[1]
    rec = torch.full((B,), -7, dtype=torch.int64, device=cuda)
    ids, x, y = _m().click_batch(torch.from_numpy(cat.view(np.int32)).to(cuda), torch.from_numpy(dense).to(cuda),
                                 torch.from_numpy(label).to(cuda), torch.from_numpy(stats).to(cuda), n, B, S, nd, V,
                                 draw, Bg, staged, rec)
    assert ids.dtype == torch.int64 and x.dtype == torch.float32 and y.dtype == torch.float32
    assert tuple(ids.shape) == (B, S) and tuple(x.shape) == (B, nd) and tuple(y.shape) == (B,)
    return ids.cpu(), x.cpu(), y.cpu(), rec.cpu().numpy()


def _check(arrays, n, B, V, stream, m, rank, world, cuda):
    """Both routes of one batch against click_batch_ref; returns the drawn records."""
    from paddle_operator_amd.data import click_batch_ref, record_index
    cat, dense, label, stats = arrays
    want_r = record_index(SEED, stream, m, rank, B, n, world * B)
    want = click_batch_ref(cat, dense, label, stats, want_r, V)
    ids, x, y, rec = _launch(arrays, n, B, V, (SEED, stream, m, rank), world * B, cuda)
    assert np.array_equal(rec, want_r), (stream, m, rank)
    assert torch.equal(ids, want[0]) and torch.equal(_bits(x), _bits(want[1])) and torch.equal(y, want[2]), (stream, m)
    # the staged route: the same draw over the gathered records (a pad row's entry is never read)
    g = np.where(want_r >= 0, want_r, 0)
    staged = (np.ascontiguousarray(cat[g]), np.ascontiguousarray(dense[g]), np.ascontiguousarray(label[g]), stats)
    ids_s, x_s, y_s, rec_s = _launch(staged, n, B, V, (SEED, stream, m, rank), world * B, cuda, staged=True)
    assert torch.equal(ids_s, ids) and torch.equal(_bits(x_s), _bits(x)) and torch.equal(y_s, y)
    assert np.array_equal(rec_s, rec)
    ws = click_batch_ref(*staged[:3], stats, want_r, V, staged=True)
    assert torch.equal(ws[0], want[0]) and torch.equal(_bits(ws[1]), _bits(want[1])) and torch.equal(ws[2], want[2])
    return rec, ids


# ----------------------------------------------------------------------------- the kernel, bit for bit
@pytest.mark.parametrize("S,nd,n,B,V", [
    (26, 13, 37, 64, 1000),      # more rows than records: duplicates
    (1, 1, 1, 1, 1),             # degenerate: every id 0
    (70, 70, 5, 5, 3),           # more columns than a wave; B no multiple of the rows per workgroup
    (26, 13, 9, 257, 2**31),     # ids above 2^32: 64-bit id arithmetic
    (26, 13, 9, 257, 2**31 - 1),
])
def test_click_batch_matches_the_reference_bit_for_bit(cuda, S, nd, n, B, V):
    arrays = _set(n, S, nd, S * 1000 + B)
    for stream, m, rank in DRAWS:
        rec, ids = _check(arrays, n, B, V, stream, m, rank, 4, cuda)
        if stream == 0:
            assert rec.min() >= 0 and rec.max() < n
            if B > n:
                assert len(np.unique(rec)) < B
        lo = torch.arange(S, dtype=torch.int64) * V
        live = torch.from_numpy(rec >= 0)
        assert ((ids >= lo) & (ids < lo + V))[live].all() and (ids[~live] == -1).all()
    if V == 1:
        assert not ids.any()
    if V >= 2**31 - 1:
        assert int(ids.max()) > 2**32


def test_dense_edges_and_cat_extremes(cuda):
    """Every edge value under every pair of stats (column k of the set uses pair k), cat 0 and
    0xFFFFFFFF; the evaluation stream reads the records in order and pads the eighth row."""
    from paddle_operator_amd.data import dense_norm
    from test_click_data_cpu import py_dense, py_hash
    n, nd, S = len(DENSE_EDGES), len(STATS_EDGES), 3
    dense = np.tile(np.array(DENSE_EDGES, dtype=np.int64).astype(np.int32)[:, None], (1, nd))
    stats = np.array(STATS_EDGES, dtype=np.float32).T.copy()  # [2, nd]
    cat = np.zeros((n, S), dtype=np.uint32)
    cat[1::2] = 0xFFFFFFFF
    cat[2, 1] = 0x80000000
    arrays = (cat, dense, np.arange(n, dtype=np.uint8) % 2, stats)
    for V in (1000, 2**31):
        ids, x, y, rec = _launch(arrays, n, 8, V, (SEED, 1, 0, 0), 8, cuda)
        assert rec.tolist() == list(range(n)) + [-1]
        want = np.array([[py_dense(int(v), *STATS_EDGES[k]) for k in range(nd)] for v in DENSE_EDGES], dtype=np.float32)
        assert np.array_equal(x[:n].numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(x[:n].numpy().view(np.uint32), dense_norm(dense, stats).view(np.uint32))
        assert not _bits(x)[0].any() and not _bits(x)[n].any()  # missing and pad: +0.0
        assert ids[:n].tolist() == [[py_hash(int(c), s, V) for s, c in enumerate(row)] for row in cat]
        assert y.tolist() == [0.0, 1.0] * 3 + [0.0, -1.0] and (ids[n] == -1).all()
    _check(arrays, n, 8, 1000, 0, 5, 1, 2, cuda)


@pytest.mark.parametrize("n", [3, 2**31 - 1])
def test_draw_only_64bit(cuda, n):
    from paddle_operator_amd.data import record_index
    B, rank = 257, 3  # one more row than a block of the records kernel
    for stream, m in ((0, 0), (0, 2**32 - 1), (0, 2**32 + 3), (1, 0), (1, 2088991)):
        out = torch.full((B,), -7, dtype=torch.int64, device=cuda)
        assert _m().click_batch(None, None, None, None, n, B, 26, 13, 1000, (SEED, stream, m, rank), 4 * B, False,
                                out) is None
        want = record_index(SEED, stream, m, rank, B, n, 4 * B)
        assert np.array_equal(out.cpu().numpy(), want), (stream, m)
    if n > 3:
        # stream 1 at m = 2 088 991: i = m·4B + 3B + j = 2 147 483 519 + j runs past n inside this rank
        assert (want >= 0).any() and (want < 0).any()
        assert int(record_index(SEED, 0, 0, rank, B, n).max()) > 2**30  # draws that need the high word


def test_evaluation_stream_pads_and_covers(cuda):
    n, B, world = 11, 4, 2
    arrays = _set(n, 26, 13, 3)
    seen = []
    for m in range(2):
        for rank in range(world):
            rec, ids = _check(arrays, n, B, 1000, 1, m, rank, world, cuda)
            assert rec.tolist() == [i if i < n else -1 for i in range(m * world * B + rank * B,
                                                                      m * world * B + rank * B + B)]
            seen += [i for i in rec.tolist() if i >= 0]
    assert sorted(seen) == list(range(n))


# ----------------------------------------------------------------------------- both routes of ClickStream
def test_staged_and_resident_routes_agree(cuda, tmp_path):
    from paddle_operator_amd.data import EVAL_STREAM, ClickStream
    n, S, nd, B, V = 13, 26, 13, 4, 1000
    cat, dense, label, stats = write_clicks(tmp_path, n, S, nd, seed=11)
    kw = dict(seed=SEED, rank=1, world=2)
    dev = ClickStream(str(tmp_path), B, S, nd, V, cuda, device_gb=1.0, **kw)
    host = ClickStream(str(tmp_path), B, S, nd, V, cuda, device_gb=0.0, **kw)
    assert (dev.placement, host.placement) == ("device", "host")
    try:
        for m in (0, 1, 2, 3, 1000, 1001, 2):  # four consecutive batches, a jump ahead, a jump back
            d, h, w = dev.batch(m), host.batch(m), dev.host_batch(m)
            assert all(t.is_cuda for t in d + h)
            for k in range(3):
                assert torch.equal(d[k], h[k]) and torch.equal(d[k].cpu(), w[k]), (m, k)
            assert torch.equal(_bits(d[1]), _bits(h[1])) and torch.equal(_bits(d[1]).cpu(), _bits(w[1])), m
        ev = ClickStream(str(tmp_path), B, S, nd, V, cuda, device_gb=0.0, stream=EVAL_STREAM, **kw)
        try:
            assert ev.batches_per_epoch() == 2
            ids, x, y = ev.batch(1)  # global rows 12 … 15 of 13 records
            w = ev.host_batch(1)
            assert y.tolist() == [float(label[12]), -1.0, -1.0, -1.0] == w[2].tolist()
            assert torch.equal(ids.cpu(), w[0]) and torch.equal(_bits(x).cpu(), _bits(w[1]))
            assert (ids[1:] == -1).all() and not _bits(x)[1:].any()
        finally:
            ev.close()
    finally:
        dev.close()
        host.close()


# ----------------------------------------------------------------------------- the contract
def test_click_batch_rejects_what_it_cannot_run(cuda):
    """Every refusal is raised by the binding's checks, before a launch; the tensors are empty."""
    e32 = torch.empty(0, dtype=torch.int32, device=cuda)
    e8, ef = torch.empty(0, dtype=torch.uint8, device=cuda), torch.empty(0, dtype=torch.float32, device=cuda)
    rec = torch.empty(4, dtype=torch.int64, device=cuda)

    def call(n=10, B=4, S=26, nd=13, V=1000, draw=(SEED, 0, 0, 0), Bg=4, sets=(None, None, None, None), out=rec):
        return _m().click_batch(*sets, n, B, S, nd, V, draw, Bg, False, out)
    assert call() is None  # the base call of the cases below is accepted
    for kw in (dict(V=0), dict(V=2**31 + 1), dict(draw=(SEED, 2, 0, 0)), dict(B=2**16, S=2**15, Bg=2**16),
               dict(B=2**16, S=2**15, Bg=2**16, sets=(e32, e32, e8, ef)), dict(n=0), dict(n=2**31),
               dict(draw=(SEED, 0, 0, 2**30)), dict(Bg=2), dict(Bg=2**31 + 4),
               dict(sets=(e32, e32, e8, ef)),  # a set that does not hold n records
               dict(out=None)):  # nothing to write
        with pytest.raises(RuntimeError):
            call(**kw)


# ----------------------------------------------------------------------------- the trainer
def test_trainer_evaluate_matches_a_recount(cuda, tmp_path):
    import torch.nn.functional as F

    from paddle_operator_amd.models.wide_deep import WideDeepConfig
    from paddle_operator_amd.ops import ctr as ctr_ops
    from paddle_operator_amd.workloads.ctr import CTRTrainer, auc_from_scores
    _, _, _, stats = write_clicks(tmp_path / "train", 300, 26, 13, seed=1)
    write_clicks(tmp_path / "val", 100, 26, 13, seed=2)
    tr = CTRTrainer(WideDeepConfig(vocab_per_slot=1000, model="deepfm"), 64, cuda, data_seed=SEED,
                    data=str(tmp_path / "train"), val_data=str(tmp_path / "val"))
    try:
        assert tr.train.placement == tr.val.placement == "device" and np.array_equal(tr.val.stats, stats)
        for _ in range(3):
            tr.step()
        ev = tr.evaluate(0)
        assert set(ev) == {"val_loss", "auc", "records"} and ev["records"] == 100
        z, y = [], []
        with torch.no_grad():
            for m in range(2):
                ids, dense, label = (t.to(cuda) for t in tr.val.host_batch(m))
                X, ws, fmt, _ = ctr_ops.ctr_lookup(ids, dense, tr.deep, tr.wide, tr.fm, tr.ldx)
                z.append(tr.tower.logit_from_lookup(X[:, :tr.K], ws, fmt))
                y.append(label)
        z, y = torch.cat(z), torch.cat(y)
        assert int((y < 0).sum()) == 28
        z, y = z[y >= 0], y[y >= 0]
        u, pairs = auc_from_scores(z, y).tolist()
        assert ev["val_loss"] == float(F.binary_cross_entropy_with_logits(z, y, reduction="sum").double()) / 100
        assert ev["auc"] == u / pairs
    finally:
        tr.close()


def test_ctr_launcher_data_resume_is_bit_exact(cuda, tmp_path):
    """4 steps straight = 2 steps, checkpoint, 2 steps resumed, on a click directory: the tables,
    the accumulators and the tower bit for bit; the records name the directories."""
    import json

    from test_ctr_gpu import _launch as launch, assert_same_state
    from paddle_operator_amd.utils import checkpoint as ckpt
    write_clicks(tmp_path / "train", 500, 26, 13, seed=1)
    write_clicks(tmp_path / "val", 70, 26, 13, seed=2)
    train, val = str(tmp_path / "train"), str(tmp_path / "val")
    base = ["--workload", "deepfm", "--tiny", "--log-every", "2", "--data", train, "--val-data", val, "--data-seed", "7",
            "--eval-every", "4", "--vocab-per-slot", "500"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    launch(base + ["--steps", "4", "--ckpt-dir", a], tmp_path / "a.log")
    launch(base + ["--steps", "2", "--ckpt-dir", b], tmp_path / "b1.log")
    launch(base + ["--steps", "4", "--ckpt-dir", b], tmp_path / "b2.log")
    assert "resumed from step 2" in open(tmp_path / "b2.log").read()
    sa, step_a = ckpt.load_latest(a)
    sb, step_b = ckpt.load_latest(b)
    assert step_a == step_b == 4 and sa["model"]["deep_emb.weight"].shape[0] == 26 * 500
    assert_same_state(sa, sb)
    assert float(sa["model"]["wide.weight"].abs().max()) > 0  # trained rows

    def rec(log, tag):
        return [json.loads(l[len(tag) + 1:]) for l in open(log).read().splitlines() if l.startswith(tag + " ")]
    ev_a, ev_b = rec(tmp_path / "a.log", "PDO_EVAL"), rec(tmp_path / "b2.log", "PDO_EVAL")
    assert ev_a == ev_b and ev_a[0]["step"] == 4 and ev_a[0]["records"] == 70
    done = rec(tmp_path / "a.log", "PDO_DONE")[0]
    assert (done["data"], done["val_data"], done["vocab_per_slot"]) == (train, val, 500)
    assert done["val_loss"] == ev_a[0]["val_loss"]


@pytest.mark.parametrize("model", ["wide_deep", "deepfm"])
def test_both_models_learn_the_planted_rule(cuda, tmp_path, model):
    """60 steps of batch 256 on the 4096 training records: the held-out loss falls below its
    step-0 value and the held-out AUC reaches 0.9 (the CPU reference path reaches 0.99)."""
    from paddle_operator_amd.models.wide_deep import WideDeepConfig
    from paddle_operator_amd.workloads.ctr import CTRTrainer
    train, val = learnable_clicks(tmp_path)
    tr = CTRTrainer(WideDeepConfig(vocab_per_slot=1000, model=model), 256, cuda, data=train, val_data=val)
    try:
        before = tr.evaluate(0)
        for _ in range(60):
            tr.step()
        after = tr.evaluate(0)
    finally:
        tr.close()
    print(f"click-learn | {model} | before {before} | after {after}")
    assert before["records"] == after["records"] == 1000
    assert after["val_loss"] < before["val_loss"] and after["auc"] >= 0.9, (before, after)
