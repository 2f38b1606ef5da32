"""Click directories on the CPU: the record draw, the slot hash and the dense normalise against
independent plain-Python implementations, the evaluation stream's coverage, the format checks, the
Criteo converter, the launcher's flags and the CTR trainer end to end (replay, checkpoint and
resume, evaluate) on directories written under ``tmp_path``.

Every comparison with a reference is bit for bit.  The writers of this file (``write_clicks``,
``learnable_clicks``) are shared with the GPU file.
"""
import struct

import numpy as np
import pytest
import torch

from paddle_operator_amd import data as D
from paddle_operator_amd.models.wide_deep import WideDeepConfig

SEED = 0xFEDC_BA98_7654_3210
MISSING = -(1 << 31)
DENSE_EDGES = (MISSING, MISSING + 1, -1, 0, 1, 2**24 + 1, 2**31 - 1)
STATS_EDGES = ((0.0, 1.0), (-5.0, 600.0), (3.0, 64000.0), (0.5, 3.0))


def write_clicks(path, n, S, nd, seed=0, stats=None, missing=0.2):
    """A random click directory; returns ``(cat, dense, label, stats)`` as written."""
    rng = np.random.default_rng(seed)
    path.mkdir(parents=True, exist_ok=True)
    cat = rng.integers(0, 2**32, (n, S), dtype=np.uint64).astype(np.uint32)
    cat[rng.random((n, S)) < 0.1] = 0
    dense = rng.integers(-50, 5000, (n, nd)).astype(np.int32)
    dense[rng.random((n, nd)) < missing] = MISSING
    label = rng.integers(0, 2, n).astype(np.uint8)
    if stats is None:
        stats = np.stack([np.full(nd, -50.0), rng.integers(1, 6000, nd).astype(np.float64)]).astype(np.float32)
    for name, a in (("cat", cat), ("dense", dense), ("label", label), ("dense_stats", stats)):
        np.save(path / f"{name}.npy", a)
    return cat, dense, label, stats


def learnable_clicks(path, S=26, nd=13):
    """The learnability fixture: 5096 records from ``default_rng(1)``, the first 4096 written to
    ``path/train``, the rest to ``path/val``.  Per slot 40 distinct random uint32 values drawn
    uniformly; dense uniform integers in [0, 100), 10 % missing; stats (0, 99); label =
    [2·(index of slot 0's value is odd) + dense₀/100 − 1.5 + 0.1·N(0, 1) > 0], missing dense₀ as 0."""
    rng = np.random.default_rng(1)
    n, cut = 5096, 4096
    values = np.stack([rng.choice(2**32, 40, replace=False) for _ in range(S)]).astype(np.uint32)  # [S, 40]
    pick = rng.integers(0, 40, (n, S))
    cat = values[np.arange(S)[None, :], pick]
    raw = rng.integers(0, 100, (n, nd))
    gone = rng.random((n, nd)) < 0.1
    d0 = np.where(gone[:, 0], 0, raw[:, 0]) / 100.0
    label = (2.0 * (pick[:, 0] % 2) + d0 - 1.5 + 0.1 * rng.standard_normal(n) > 0).astype(np.uint8)
    dense = np.where(gone, MISSING, raw).astype(np.int32)
    stats = np.stack([np.zeros(nd), np.full(nd, 99.0)]).astype(np.float32)
    for name, sl in (("train", slice(0, cut)), ("val", slice(cut, n))):
        (path / name).mkdir(parents=True, exist_ok=True)
        for f, a in (("cat", cat[sl]), ("dense", dense[sl]), ("label", label[sl])):
            np.save(path / name / f"{f}.npy", np.ascontiguousarray(a))
        np.save(path / name / "dense_stats.npy", stats)
    return str(path / "train"), str(path / "val")


# ----------------------------------------------------------------------------- plain-Python references
M32 = 0xFFFFFFFF


def py_philox(c, key):
    c, (k0, k1) = list(c), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def py_record(seed, stream, m, g, n, Bglobal):
    if stream == 1:
        i = (m & M32) * Bglobal + g
        return i if i < n else -1
    w = py_philox((g, 0, stream, m & M32), (seed & M32, (seed >> 32) & M32))
    return ((w[1] << 32) | w[0]) % n


def py_hash(c, s, V):
    h = c ^ (((s + 1) * 0x9E3779B9) & M32)
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return s * V + ((h * V) >> 32)


def f32(x: float) -> float:
    """The float32 nearest to the double ``x`` (round to nearest even), as a double."""
    return struct.unpack("f", struct.pack("f", x))[0]


def py_dense(v, mn, df):
    """fl(fl(float(v) − min) / diff): every operation in double, then rounded once to float32 — a
    double holds the exact sum and a quotient that rounds to float32 as the exact one does."""
    if v == MISSING:
        return 0.0
    return f32(f32(f32(float(v)) - mn) / df)


# ----------------------------------------------------------------------------- draw and hash
def test_record_index_matches_plain_python():
    for n in (1, 3, 37, 2**31 - 1):
        for m, rank, B in ((0, 0, 5), (2**32 + 3, 3, 4), (2**32 - 1, 1, 3)):
            got = D.record_index(SEED, 0, m, rank, B, n)
            want = [py_record(SEED, 0, m, rank * B + j, n, 4 * B) for j in range(B)]
            assert got.dtype == np.int64 and got.tolist() == want, (n, m)
            assert got.min() >= 0 and got.max() < n
            ev = D.record_index(SEED, 1, m, rank, B, n, 4 * B)
            assert ev.tolist() == [py_record(SEED, 1, m, rank * B + j, n, 4 * B) for j in range(B)], (n, m)
    assert not np.array_equal(D.record_index(SEED, 0, 0, 0, 64, 10**6), D.record_index(SEED + 1, 0, 0, 0, 64, 10**6))
    assert not np.array_equal(D.record_index(SEED, 0, 0, 0, 64, 10**6), D.record_index(SEED, 0, 1, 0, 64, 10**6))


@pytest.mark.parametrize("V", [1, 3, 1000, 2**31 - 1, 2**31])
def test_hash_rows_matches_plain_python(V):
    rng = np.random.default_rng(V % 1000)
    S = 70
    cat = rng.integers(0, 2**32, (40, S), dtype=np.uint64).astype(np.uint32)
    cat[0], cat[1], cat[2] = 0, 0x80000000, 0xFFFFFFFF
    ids = D.hash_rows(cat, V)
    assert ids.dtype == np.int64 and ids.shape == cat.shape
    for s in (0, 25, 69):
        assert ids[:, s].tolist() == [py_hash(int(c), s, V) for c in cat[:, s]], s
    lo = np.arange(S, dtype=np.int64) * V
    assert (ids >= lo).all() and (ids < lo + V).all()
    for bad in (0, 2**31 + 1):
        with pytest.raises(ValueError):
            D.hash_rows(cat, bad)


def test_hash_spreads_and_separates_slots():
    cat = np.tile(np.arange(5000, dtype=np.uint32)[:, None], (1, 2))
    ids = D.hash_rows(cat, 1 << 20)
    assert len(np.unique(ids[:, 0])) > 4950  # 5000 values in 2^20 rows: about 12 expected collisions
    assert not np.array_equal(ids[:, 0], ids[:, 1] - (1 << 20))  # the salt: slots hash the same value apart


def test_dense_norm_edges_are_float32_exact():
    raw = np.array(DENSE_EDGES, dtype=np.int64).astype(np.int32)
    for mn, df in STATS_EDGES:
        stats = np.array([[mn] * 2, [df] * 2], dtype=np.float32)
        got = D.dense_norm(np.stack([raw, raw], axis=1), stats)
        assert got.dtype == np.float32 and got.shape == (len(raw), 2)
        want = np.array([py_dense(int(v), mn, df) for v in raw], dtype=np.float32)
        assert np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32)), (mn, df)
        assert got[0, 0].view(np.uint32) == 0  # missing: +0.0, not −0.0
    rng = np.random.default_rng(0)
    raw = rng.integers(-2**31, 2**31, 2000).astype(np.int32)
    stats = np.array([[-12345.678], [987.125]], dtype=np.float32)
    want = np.array([py_dense(int(v), float(stats[0, 0]), float(stats[1, 0])) for v in raw], dtype=np.float32)
    assert np.array_equal(D.dense_norm(raw[:, None], stats)[:, 0].view(np.uint32), want.view(np.uint32))


# ----------------------------------------------------------------------------- streams
@pytest.mark.parametrize("n,world,B", [(11, 2, 4), (1, 1, 3), (64, 4, 16)])
def test_evaluation_visits_every_record_once(tmp_path, n, world, B):
    cat, dense, label, stats = write_clicks(tmp_path, n, 3, 2, seed=n)
    seen = []
    for rank in range(world):
        s = D.ClickStream(str(tmp_path), B, 3, 2, 50, "cpu", seed=SEED, stream=D.EVAL_STREAM, rank=rank, world=world)
        assert s.placement == "cpu" and s.batches_per_epoch() == -(-n // (world * B))
        for m in range(s.batches_per_epoch()):
            rec = s.records(m)
            ids, x, y = s.batch(m)
            pad = rec < 0
            assert (ids[pad] == -1).all() and (y[pad] == -1).all() and not x[pad].view(torch.int32).any()
            live = rec[~pad]
            assert torch.equal(ids[~pad], torch.from_numpy(D.hash_rows(cat[live], 50)))
            assert torch.equal(x[~pad], torch.from_numpy(D.dense_norm(dense[live], stats)))
            assert torch.equal(y[~pad], torch.from_numpy(label[live].astype(np.float32)))
            seen += live.tolist()
        assert (s.records(s.batches_per_epoch()) == -1).all()
    assert sorted(seen) == list(range(n))


def test_training_batch_does_not_depend_on_the_split(tmp_path):
    write_clicks(tmp_path, 37, 4, 3, seed=1)

    def stream(B, rank, world, **kw):
        return D.ClickStream(str(tmp_path), B, 4, 3, 1000, "cpu", seed=SEED, rank=rank, world=world, **kw)
    for m in (0, 5, 2**32 + 1):
        whole = stream(8, 0, 1).batch(m)
        halves = [stream(4, r, 2).batch(m) for r in (0, 1)]
        for k in range(3):
            assert torch.equal(whole[k], torch.cat([h[k] for h in halves]))
    ids, x, y = stream(8, 0, 1).batch(0)
    assert ids.dtype == torch.int64 and x.dtype == torch.float32 and y.dtype == torch.float32
    assert tuple(ids.shape) == (8, 4) and tuple(x.shape) == (8, 3) and tuple(y.shape) == (8,)
    # another directory's stats replace the stream's own
    other = np.array([[1.0] * 3, [2.0] * 3], dtype=np.float32)
    assert torch.equal(stream(8, 0, 1, stats=other).batch(0)[1],
                       torch.from_numpy(D.dense_norm(np.load(tmp_path / "dense.npy")[stream(8, 0, 1).records(0)], other)))


def test_staging_gather_fills_the_drawn_records(tmp_path):
    """The host-staged route's gather, which needs no GPU: live rows hold their records, pad rows
    are left alone (evaluation batch 1 of 2 is 4 records and 3 pad rows, batch 2 pad rows only)."""
    n, S, nd, B = 11, 3, 2, 7
    cat, dense, label, _ = write_clicks(tmp_path, n, S, nd, seed=3)
    for stream, m, pads in ((D.TRAIN_STREAM, 0, 0), (D.TRAIN_STREAM, 9, 0), (D.EVAL_STREAM, 0, 0), (D.EVAL_STREAM, 1, 3),
                            (D.EVAL_STREAM, 2, 7)):
        s = D.ClickStream(str(tmp_path), B, S, nd, 50, "cpu", seed=SEED, stream=stream)
        rec = s.records(m)
        live = rec >= 0
        assert int((~live).sum()) == pads
        outs = (np.full((B, S), 7, np.uint32), np.full((B, nd), 7, np.int32), np.full(B, 7, np.uint8))
        s._gather(m, outs)
        for o, a in zip(outs, (cat, dense, label)):
            assert np.array_equal(o[live], a[rec[live]]) and (o[~live] == 7).all(), (stream, m)


def test_open_clicks_rejects_with_the_file_name(tmp_path):
    S, nd, n = 3, 2, 6
    cat, dense, label, stats = write_clicks(tmp_path, n, S, nd)
    assert D.open_clicks(str(tmp_path), S, nd)[0].shape == (n, S)
    good = {"cat": cat, "dense": dense, "label": label, "dense_stats": stats}
    bad_stats = [stats.copy() for _ in range(3)]
    bad_stats[0][0, 1] = np.inf
    bad_stats[1][1, 0] = np.nan
    bad_stats[2][1, 1] = 0.0
    cases = [("cat", cat.astype(np.int32)), ("cat", cat.astype(np.uint64)), ("dense", dense.astype(np.int64)),
             ("label", label.astype(np.int8)), ("dense_stats", stats.astype(np.float64)),
             ("cat", cat[:, :2].copy()), ("dense", np.concatenate([dense, dense], 1)),  # widths
             ("dense", dense[:-1].copy()), ("label", label[:-1].copy()),  # unequal n
             ("cat", np.asfortranarray(cat)), ("dense", np.asfortranarray(dense)),  # not C order
             ("label", np.where(np.arange(n) == 2, 2, label).astype(np.uint8)),
             ("dense_stats", stats[:, :1].copy())] + [("dense_stats", s) for s in bad_stats]
    for name, arr in cases:
        np.save(tmp_path / f"{name}.npy", arr)
        with pytest.raises(ValueError, match=f"{name}.npy"):
            D.open_clicks(str(tmp_path), S, nd)
        np.save(tmp_path / f"{name}.npy", good[name])
    D.open_clicks(str(tmp_path), S, nd)
    with pytest.raises(ValueError, match="cat.npy"):
        D.open_clicks(str(tmp_path), S + 1, nd)  # the model's n_sparse
    with pytest.raises(ValueError, match="dense.npy"):
        D.open_clicks(str(tmp_path), S, nd + 1)


# ----------------------------------------------------------------------------- converter
def test_converter_round_trip(tmp_path):
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [(1, [5, "", -3], ["0000000a", "ffffffff", ""]),
            (0, [7, 2, ""], ["", "80000000", "1"]),
            (0, ["", 2, 4], ["deadbeef", "", "00000000"]),
            (1, [5, "", 4], ["a", "b", "c"]),
            (0, [0, 9, -3], ["12345678", "9abcdef0", "0fedcba9"]),
            (1, [1, "", ""], ["", "", ""])]
    tsv = tmp_path / "log.txt"
    tsv.write_text("".join("\t".join([str(y)] + [str(v) for v in d] + c) + "\n" for y, d, c in rows))
    tool = [sys.executable, os.path.join(repo, "tools", "criteo_to_clicks.py")]
    out = tmp_path / "train"
    subprocess.run(tool + [str(tsv), str(out), "--n-dense", "3", "--n-sparse", "3", "--chunk", "4"], check=True,
                   timeout=120)
    cat, dense, label, stats = D.open_clicks(str(out), 3, 3)
    assert label.tolist() == [y for y, _, _ in rows]
    assert dense.tolist() == [[MISSING if v == "" else v for v in d] for _, d, _ in rows]
    assert cat.tolist() == [[int(t, 16) if t else 0 for t in c] for _, _, c in rows]
    # min, and max − min with 0 replaced by 1 (feature 1 is 2 or 9; feature 0 spans 0 … 7)
    assert stats.tolist() == [[0.0, 2.0, -3.0], [7.0, 7.0, 7.0]]
    one = tmp_path / "one.txt"
    one.write_text("1\t4\t\t4\ta\tb\tc\n0\t4\t\t\ta\tb\tc\n")  # a constant feature, an absent one
    subprocess.run(tool + [str(one), str(tmp_path / "one"), "--n-dense", "3", "--n-sparse", "3"], check=True, timeout=120)
    assert np.load(tmp_path / "one" / "dense_stats.npy").tolist() == [[4.0, 0.0, 4.0], [1.0, 1.0, 1.0]]
    subprocess.run(tool + [str(one), str(tmp_path / "val"), "--n-dense", "3", "--n-sparse", "3", "--stats-from", str(out)],
                   check=True, timeout=120)
    assert np.array_equal(np.load(tmp_path / "val" / "dense_stats.npy"), stats)
    assert D.open_clicks(str(tmp_path / "val"), 3, 3)[0].shape == (2, 3)
    bad = tmp_path / "bad.txt"
    bad.write_text("1\t4\t\t4\ta\tb\n")
    assert subprocess.run(tool + [str(bad), str(tmp_path / "bad"), "--n-dense", "3", "--n-sparse", "3"],
                          stderr=subprocess.DEVNULL, timeout=120).returncode != 0


# ----------------------------------------------------------------------------- the trainer
@pytest.fixture
def sets(tmp_path):
    _, _, _, stats = write_clicks(tmp_path / "train", 50, 26, 13, seed=1)
    write_clicks(tmp_path / "val", 21, 26, 13, seed=2)  # its own stats differ: the trainer uses train's
    return str(tmp_path / "train"), str(tmp_path / "val")


def _trainer(sets, model="deepfm", **kw):
    from paddle_operator_amd.workloads.ctr import CTRTrainer
    return CTRTrainer(WideDeepConfig(vocab_per_slot=50, model=model), 8, "cpu", data_seed=SEED, data=sets[0],
                      val_data=sets[1], **kw)


def _same_state(a, b):
    from test_ctr_gpu import assert_same_state
    assert_same_state(a, b)


def test_trainer_draws_the_reference_batches_and_replays(sets):
    from paddle_operator_amd.workloads.ctr import EVAL_STREAM, TRAIN_STREAM
    a, b = _trainer(sets), _trainer(sets)
    assert a.train.placement == a.val.placement == "cpu"
    assert np.array_equal(a.val.stats, a.train.stats) and not np.array_equal(a.val.stats, np.load(sets[1] + "/dense_stats.npy"))
    for m in (0, 3):
        for got, want in zip(a.draw(TRAIN_STREAM, m), a.train.host_batch(m)):
            assert torch.equal(got, want)
        for got, want in zip(a.draw(EVAL_STREAM, m), a.val.host_batch(m)):
            assert torch.equal(got, want)
    la, lb = [float(a.step()) for _ in range(4)], [float(b.step()) for _ in range(4)]
    assert la == lb
    _same_state(a.state_dict(), b.state_dict())
    a.close()
    b.close()


@pytest.mark.parametrize("model", ["wide_deep", "deepfm"])
def test_trainer_resume_is_bitwise(sets, tmp_path, model):
    from paddle_operator_amd.utils import checkpoint as ckpt
    a = _trainer(sets, model)
    la = [float(a.step()) for _ in range(4)]
    b = _trainer(sets, model)
    lb = [float(b.step()) for _ in range(2)]
    ckpt.save(b.state_dict(), str(tmp_path / "ck"), 2)
    st, step = ckpt.load_latest(str(tmp_path / "ck"))
    c = _trainer(sets, model)
    c.load_state_dict(st)
    assert step == 2 and c.step_count == 2
    lb += [float(c.step()) for _ in range(2)]
    assert la == lb
    _same_state(a.state_dict(), c.state_dict())


def test_trainer_evaluate_counts_every_record(sets):
    import torch.nn.functional as F

    from paddle_operator_amd.ops import ctr as ctr_ops
    from paddle_operator_amd.workloads.ctr import CTRTrainer, auc_from_scores
    tr = _trainer(sets)
    for _ in range(2):
        tr.step()
    ev = tr.evaluate(0)
    assert set(ev) == {"val_loss", "auc", "records"} and ev["records"] == 21 and ev == tr.evaluate(0)
    assert tr.evaluate(1)["records"] == 8 and tr.evaluate(3)["records"] == 21
    # a recount from the host batches: three batches of 8, the last with 3 pad rows
    z, y = [], []
    with torch.no_grad():
        for m in range(3):
            ids, dense, label = tr.val.host_batch(m)
            X, ws, fmt, _ = ctr_ops.ctr_lookup(ids, dense, tr.deep, tr.wide, tr.fm, tr.ldx)
            z.append(tr.tower.logit_from_lookup(X[:, :tr.K], ws, fmt))
            y.append(label)
    z, y = torch.cat(z), torch.cat(y)
    assert int((y < 0).sum()) == 3
    z, y = z[y >= 0], y[y >= 0]
    u, pairs = auc_from_scores(z, y).tolist()
    assert ev["val_loss"] == float(F.binary_cross_entropy_with_logits(z, y, reduction="sum").double()) / 21
    assert ev["auc"] == u / pairs
    # without val_data the synthetic evaluation is what it was: no "records"
    assert set(CTRTrainer(WideDeepConfig(vocab_per_slot=50), 8, "cpu", data=sets[0]).evaluate(1)) == {"val_loss", "auc"}


# ----------------------------------------------------------------------------- the launcher's flags
def test_parse_args_ctr_flags(monkeypatch):
    from paddle_operator_amd.launch.run import _ctr_flags, parse_args
    for k in ("PDO_TRAIN_DATA", "PDO_VAL_DATA", "PADDLE_PSERVERS_IP_PORT_LIST"):
        monkeypatch.delenv(k, raising=False)
    a = parse_args(["--workload", "deepfm", "--data", "d", "--val-data", "v", "--eval-every", "5", "--vocab-per-slot",
                    "777", "--data-device-gb", "0.5"])
    assert (a.data, a.val_data, a.vocab_per_slot, a.data_device_gb, a.eval_batches) == ("d", "v", 777, 0.5, 0)
    assert _ctr_flags(a) == {"data": "d", "val_data": "v", "vocab_per_slot": 777}
    assert parse_args(["--workload", "wide_deep", "--val-data", "v", "--eval-batches", "3"]).eval_batches == 3
    # with no new flag: today's namespace, and nothing added to the records
    b = parse_args(["--workload", "wide_deep", "--eval-every", "10"])
    assert (b.data, b.val_data, b.vocab_per_slot, b.eval_batches, b.eval_every, b.lr, b.lr_given, b.sparse_lr,
            b.data_seed, b.data_device_gb) == ("", "", None, 8, 10, 1e-3, False, 0.05, 0, 8.0)
    assert _ctr_flags(b) == {}
    g = parse_args(["--workload", "gpt2"])
    assert g.eval_batches == 8 and g.vocab_per_slot is None and parse_args(["--workload", "resnet50"]).eval_batches == 0
    # the two errors
    with pytest.raises(SystemExit):
        parse_args(["--workload", "wide_deep", "--data", "d", "--eval-every", "10"])
    monkeypatch.setenv("PADDLE_PSERVERS_IP_PORT_LIST", "10.0.0.1:8000")
    with pytest.raises(SystemExit):
        parse_args(["--workload", "deepfm", "--data", "d"])
    assert parse_args(["--workload", "deepfm"]).data == ""  # a PS job without the flag is untouched
    monkeypatch.delenv("PADDLE_PSERVERS_IP_PORT_LIST")
    with pytest.raises(SystemExit):
        parse_args(["--workload", "gpt2", "--vocab-per-slot", "10"])
